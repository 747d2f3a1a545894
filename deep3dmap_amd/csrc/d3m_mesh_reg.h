// d3m_mesh_reg.h -- shape regularisers of an indexed mesh: the uniform Laplacian, the edge-length and the normal-consistency
// term of vertices [B, V, 3], value and gradient, over a topology built once per faces tensor (d3m_mesh_topology,
// neural_renderer/mesh_regularizers.py).  Everything is a gather: a vertex reads its own neighbour row and its own wing row
// in item order and stores its gradient once.  No float atomics; every sum that crosses lanes or workgroups has a fixed
// order, and no workgroup waits for another (the value is finished by a launch of one workgroup per vertex set).
//
//   Laplacian   delta_v = x_v - mean of N(v) (0 where deg v = 0);  L = (1/V) sum |delta_v|^2;
//               dL/dx_v = (2/V) (delta_v - sum over u in N(v) of delta_u / deg u)        (the relation is symmetric)
//   edge        l = |x_a - x_b|;  L = (1/E) sum (l - l0)^2;  dL/dx_a = (2/E) (l - l0) (x_a - x_b) / l, 0 where l = 0;
//               the value of an edge is counted at its lower endpoint
//   normal      per wing record (a, b, c, d): n0 = (b-a) x (c-a), n1 = -(b-a) x (d-a), L = (1/P) sum (1 - cos(n0, n1)),
//               0 where a normal vanishes; the value of a record is counted at role 0 (a)
//
// Passes: k_mesh_reg_delta (delta and 1/deg of every vertex into scratch; only with the Laplacian), k_mesh_reg_rows (the
// gathered gradient and the workgroup's value), k_mesh_reg_finish.  Rows of more than long_row items (a pole, a fan apex)
// go through the chunks of d3m_row_gather.h, which states the order, in both directions: k_mesh_reg_mean_chunks (the hub's
// neighbour sum for delta) and k_mesh_reg_row_chunks (its gathered gradient and value).
#pragma once
#include "d3m_aux.h"
#include "d3m_row_gather.h"

namespace d3m {

constexpr int MR_BLOCK = RG_BLOCK;

struct MeshRegArgs {
    CsrRows nbr, wing;          // the neighbour CSR and the wing CSR, V rows each
    const int32_t* wings;       // [P, 4] (a, b, c, d), 16-byte aligned
    int V;
    const float* x;             // [B, V, 3]
    float4* delta;              // [B, V] (delta, 1/deg); NULL without the Laplacian
    float* mean_partials;       // [B, num_nbr_chunks, 3]
    float* row_partials;        // [B, num_nbr_chunks + num_wing_chunks, 4] (gradient, value)
    float* value_partials;      // [B, workgroups of k_mesh_reg_rows]
    float c_lap, c_edge, c_nc;  // weight / count of each term (0: the term is off)
    float edge_target;
    const float* grad_scale;    // [B] or NULL (1)
    float* loss_out;            // [B]
    float* grad;                // [B, V, 3] or NULL (value only)
    int accumulate;
};

struct mr3 { float x, y, z; };
__device__ __forceinline__ mr3 mr_load(const float* __restrict__ p, int v) {
    const float* q = p + (size_t)v * 3;
    return {q[0], q[1], q[2]};
}
__device__ __forceinline__ mr3 mr_sub(mr3 a, mr3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ mr3 mr_cross(mr3 a, mr3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float mr_dot(mr3 a, mr3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }

// One item of v's neighbour row: what neighbour u adds to v's gradient (x, y, z) and to the value (w).
__device__ __forceinline__ float4 mr_nbr_term(const MeshRegArgs& a, const float* __restrict__ x, const float4* __restrict__ delta,
                                              int v, mr3 xv, int u) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.c_lap > 0.f && a.grad) {
        const float4 du = delta[u];
        const float s = -2.0f * a.c_lap * du.w;
        r.x = s * du.x; r.y = s * du.y; r.z = s * du.z;
    }
    if (a.c_edge > 0.f) {
        const mr3 d = mr_sub(xv, mr_load(x, u));
        const float len = sqrtf(mr_dot(d, d));
        const float off = len - a.edge_target;
        if (len > 0.f) {
            const float s = 2.0f * a.c_edge * off / len;
            r.x += s * d.x; r.y += s * d.y; r.z += s * d.z;
        }
        if (u > v) r.w = a.c_edge * off * off;
    }
    return r;
}

// One item (4 p + role) of v's wing row.
__device__ __forceinline__ float4 mr_wing_term(const MeshRegArgs& a, const float* __restrict__ x, int item) {
    const int p = item >> 2, role = item & 3;
    const int4 w = reinterpret_cast<const int4*>(a.wings)[p];
    const mr3 xa = mr_load(x, w.x);
    const mr3 e = mr_sub(mr_load(x, w.y), xa), u = mr_sub(mr_load(x, w.z), xa), q = mr_sub(mr_load(x, w.w), xa);
    const mr3 n0 = mr_cross(e, u), n1 = mr_cross(q, e);
    const float s0 = mr_dot(n0, n0), s1 = mr_dot(n1, n1);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (s0 > 0.f && s1 > 0.f) {
        const float i0 = 1.0f / sqrtf(s0), i1 = 1.0f / sqrtf(s1);
        const mr3 h0 = {n0.x * i0, n0.y * i0, n0.z * i0}, h1 = {n1.x * i1, n1.y * i1, n1.z * i1};
        const float c = mr_dot(h0, h1);
        // d cos / d n0 and d cos / d n1
        const mr3 g0 = {(h1.x - c * h0.x) * i0, (h1.y - c * h0.y) * i0, (h1.z - c * h0.z) * i0};
        const mr3 g1 = {(h0.x - c * h1.x) * i1, (h0.y - c * h1.y) * i1, (h0.z - c * h1.z) * i1};
        const mr3 ue = mr_cross(u, g0), we = mr_cross(g1, q);           // d cos / d e = u x g0 + g1 x q
        const mr3 ge = {ue.x + we.x, ue.y + we.y, ue.z + we.z};
        const mr3 gu = mr_cross(g0, e), gq = mr_cross(e, g1);            // d cos / d u, d cos / d q
        mr3 g;
        if (role == 0) g = {-(ge.x + gu.x + gq.x), -(ge.y + gu.y + gq.y), -(ge.z + gu.z + gq.z)};
        else if (role == 1) g = ge;
        else if (role == 2) g = gu;
        else g = gq;
        r.x = -a.c_nc * g.x; r.y = -a.c_nc * g.y; r.z = -a.c_nc * g.z;
        if (role == 0) r.w = a.c_nc * (1.0f - c);
    }
    return r;
}

__device__ __forceinline__ void mr_add(float4& acc, float4 t) { acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w; }
__device__ __forceinline__ void mr_add(float (&acc)[4], float4 t) { acc[0] += t.x; acc[1] += t.y; acc[2] += t.z; acc[3] += t.w; }

// adds the chunk sums (gradient, value) of the long row `v` onto acc
__device__ __forceinline__ void mr_add_long_row(const LongRows& t, int v, const float* __restrict__ part, float4& acc) {
    float s[4] = {acc.x, acc.y, acc.z, acc.w};
    rg_add_chunk_sums(t, rg_find_long(t, v), part, s);
    acc = make_float4(s[0], s[1], s[2], s[3]);
}

// ---- the hubs' neighbour sums: one workgroup per chunk of a long neighbour row ------------------------------------------
__global__ void __launch_bounds__(MR_BLOCK) k_mesh_reg_mean_chunks(MeshRegArgs a) {
    const int ch = blockIdx.x, b = blockIdx.y;
    const float* x = a.x + (size_t)b * a.V * 3;
    float sum[3];
    rg_chunk_sum(a.nbr.longs.chunks[ch], sum, [&](int e, float (&acc)[3]) {
        const mr3 xu = mr_load(x, a.nbr.items[e]);
        acc[0] += xu.x; acc[1] += xu.y; acc[2] += xu.z;
    });
    if (threadIdx.x == 0) {
        float* out = a.mean_partials + ((size_t)b * a.nbr.longs.n_chunks + ch) * 3;
        out[0] = sum[0]; out[1] = sum[1]; out[2] = sum[2];
    }
}

// ---- delta: one lane per vertex -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MR_BLOCK) k_mesh_reg_delta(MeshRegArgs a) {
    const int v = blockIdx.x * MR_BLOCK + threadIdx.x, b = blockIdx.y, V = a.V;
    if (v >= V) return;
    const float* x = a.x + (size_t)b * V * 3;
    const int start = a.nbr.offsets[v], end = a.nbr.offsets[v + 1], deg = end - start;
    float4 out = make_float4(0.f, 0.f, 0.f, 0.f);
    if (deg > 0) {
        const LongRows& longs = a.nbr.longs;
        float s[3] = {0.f, 0.f, 0.f};
        if (rg_is_long(longs, deg)) {
            rg_add_chunk_sums(longs, rg_find_long(longs, v), a.mean_partials + (size_t)b * a.nbr.longs.n_chunks * 3, s);
        } else {
            for (int e = start; e < end; e++) {
                const mr3 xu = mr_load(x, a.nbr.items[e]);
                s[0] += xu.x; s[1] += xu.y; s[2] += xu.z;
            }
        }
        const float inv = 1.0f / (float)deg;
        const mr3 xv = mr_load(x, v);
        out = make_float4(xv.x - s[0] * inv, xv.y - s[1] * inv, xv.z - s[2] * inv, inv);
    }
    a.delta[(size_t)b * V + v] = out;
}

// ---- the hubs' gathered gradient and value: one workgroup per chunk of a long neighbour row, then of a long wing row ----
__global__ void __launch_bounds__(MR_BLOCK) k_mesh_reg_row_chunks(MeshRegArgs a) {
    const int ch = blockIdx.x, b = blockIdx.y, V = a.V;
    const float* x = a.x + (size_t)b * V * 3;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (ch < a.nbr.longs.n_chunks) {
        const LongRows& longs = a.nbr.longs;
        const int v = rg_chunk_owner(longs, ch);
        const float4* delta = a.delta ? a.delta + (size_t)b * V : nullptr;
        const mr3 xv = mr_load(x, v);
        rg_lane_sum(longs.chunks[ch], acc, [&](int e, float (&t)[4]) { mr_add(t, mr_nbr_term(a, x, delta, v, xv, a.nbr.items[e])); });
    } else if (a.c_nc > 0.f) {
        rg_lane_sum(a.wing.longs.chunks[ch - a.nbr.longs.n_chunks], acc,
                    [&](int e, float (&t)[4]) { mr_add(t, mr_wing_term(a, x, a.wing.items[e])); });
    }
    rg_block_sum(acc);
    if (threadIdx.x == 0) {
        float* out = a.row_partials + ((size_t)b * (a.nbr.longs.n_chunks + a.wing.longs.n_chunks) + ch) * 4;
        out[0] = acc[0]; out[1] = acc[1]; out[2] = acc[2]; out[3] = acc[3];
    }
}

// ---- rows: one lane per vertex walks its neighbour row and its wing row; the workgroup stores 768 contiguous floats and
// one value partial ----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(MR_BLOCK) k_mesh_reg_rows(MeshRegArgs a) {
    __shared__ float staged[MR_BLOCK * 3];
    const int v = blockIdx.x * MR_BLOCK + threadIdx.x, b = blockIdx.y, V = a.V;
    const float* x = a.x + (size_t)b * V * 3;
    const float4* delta = a.delta ? a.delta + (size_t)b * V : nullptr;
    const int n_chunks = a.nbr.longs.n_chunks + a.wing.longs.n_chunks;
    const float* part = a.row_partials + (size_t)b * n_chunks * 4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (v < V) {
        if (a.c_lap > 0.f) {
            const float4 dv = delta[v];
            const float s = 2.0f * a.c_lap;
            acc = make_float4(s * dv.x, s * dv.y, s * dv.z, a.c_lap * (dv.x * dv.x + dv.y * dv.y + dv.z * dv.z));
        }
        if (a.c_edge > 0.f || (a.c_lap > 0.f && a.grad)) {
            const LongRows& longs = a.nbr.longs;
            const int start = a.nbr.offsets[v], end = a.nbr.offsets[v + 1];
            if (rg_is_long(longs, end - start)) {
                mr_add_long_row(longs, v, part, acc);
            } else {
                const mr3 xv = mr_load(x, v);
                for (int e = start; e < end; e++) mr_add(acc, mr_nbr_term(a, x, delta, v, xv, a.nbr.items[e]));
            }
        }
        if (a.c_nc > 0.f) {
            const LongRows& longs = a.wing.longs;
            const int start = a.wing.offsets[v], end = a.wing.offsets[v + 1];
            if (rg_is_long(longs, end - start)) {
                mr_add_long_row(longs, v, part + (size_t)a.nbr.longs.n_chunks * 4, acc);
            } else {
                for (int e = start; e < end; e++) mr_add(acc, mr_wing_term(a, x, a.wing.items[e]));
            }
        }
    }
    float value[1] = {acc.w};
    rg_block_sum(value);
    if (threadIdx.x == 0) a.value_partials[(size_t)b * gridDim.x + blockIdx.x] = value[0];
    if (!a.grad) return;
    const float scale = a.grad_scale ? a.grad_scale[b] : 1.0f;
    staged[threadIdx.x * 3 + 0] = scale * acc.x;
    staged[threadIdx.x * 3 + 1] = scale * acc.y;
    staged[threadIdx.x * 3 + 2] = scale * acc.z;
    __syncthreads();
    const long base = (long)blockIdx.x * MR_BLOCK * 3, n = (long)V * 3;
    float* g = a.grad + (size_t)b * n;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const long i = base + k * MR_BLOCK + threadIdx.x;
        if (i < n) g[i] = a.accumulate ? g[i] + staged[k * MR_BLOCK + threadIdx.x] : staged[k * MR_BLOCK + threadIdx.x];
    }
}

// ---- the value: one workgroup per vertex set adds the rows pass's partials, lane by stride in f64, then in lane order -----
__global__ void __launch_bounds__(MR_BLOCK) k_mesh_reg_finish(const float* __restrict__ value_partials, int n_partials,
                                                              float* __restrict__ loss_out, int accumulate) {
    __shared__ double lane_sum[MR_BLOCK];
    const int b = blockIdx.x;
    const float* part = value_partials + (size_t)b * n_partials;
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += MR_BLOCK) s += (double)part[i];
    lane_sum[threadIdx.x] = s;
    __syncthreads();
    for (int half = MR_BLOCK / 2; half >= 1; half >>= 1) {
        if ((int)threadIdx.x < half) lane_sum[threadIdx.x] += lane_sum[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_out[b] = accumulate ? loss_out[b] + (float)lane_sum[0] : (float)lane_sum[0];
}

}  // namespace d3m
