// d3m_set_sums.h -- a few sums per set over many elements, in two launches and one fixed tree, stated once for every
// parameter adjoint that reduces this way: the camera's parameters (d3m_camera_grad.h: a set is a view, an element a
// vertex), the light's (d3m_light_grad.h: a light row, a face), the weak-perspective pose (d3m_pose.h: a point set, a
// vertex) and the SH coefficients (d3m_smooth_shade.h: a set, a vertex).  tests/set_sums_replay.py replays it in numpy.
//
// A node names three things: N sums per element, PER_PART elements per part with at most MAX_PARTS parts per set
// (parts = set_parts(elements, PER_PART, MAX_PARTS)), and its WaveTree.  THE ORDER of set b's sum k, the same bits on every
// run:
//   1. a partial kernel runs one workgroup of SET_BLOCK lanes per (set, part); lane t of part p adds the terms of the
//      elements SET_BLOCK p + t, + SET_BLOCK parts, + 2 SET_BLOCK parts, ... in that order, from 0 (the loop is the node's:
//      it knows its terms, which elements it skips, and what else it stores from the same read);
//   2. the 64 lanes of a wave are combined by the node's WaveTree:
//        XorButterfly   v += __shfl_xor(v, off, 64), off = 32, 16, ..., 1                              (camera, light)
//        DppRows        d3m_device.h's wave_sum: inside each row of 16 lanes v += v[lane ^ 1], v += v[lane ^ 2],
//                       v += v[the lane's mirror in its half of 8], v += v[its mirror in the row]; then, with r0 .. r3
//                       the rows' sums (lanes 0, 16, 32, 48), (r0 + r1) + (r2 + r3)                       (pose, SH)
//   3. lane 0 of each wave stages its sum; after ONE barrier the part's sum is ((w0 + w1) + w2) + w3 -- it starts from
//      wave 0's value, not from 0 (0 + -0 is +0) -- stored plainly at partial[(b parts + p) STRIDE + k];
//   4. a finish kernel adds the set's parts in ascending p, from 0;
//   5. (camera, light) the finish forms a row of gradients per set; a parameter with a batch dimension takes each set's
//      row, a parameter of batch 1 the sum of the rows in ascending set order, from 0.
// No float atomics, and no workgroup waits for another: the partials go through caller-owned scratch between the launches.
#pragma once
#include "d3m_device.h"

namespace d3m {

constexpr int SET_BLOCK = 256;          // lanes of a partial workgroup: four waves

// parts of a set of `items` elements: per_part elements each, at least 1, at most max_parts (beyond that the lanes stride)
__host__ __device__ __forceinline__ int set_parts(long items, int per_part, int max_parts) {
    const long n = (items + per_part - 1) / per_part;
    return n < 1 ? 1 : (n > max_parts ? max_parts : (int)n);
}

enum class WaveTree { XorButterfly, DppRows };

// Step 2 for N components: each becomes its wave's sum, in every lane.  (Written on the array: the scalar form below,
// called per component, made the compiler schedule the row gathers' chunk kernels into 10 and 42 more VGPRs.)
template <WaveTree T, int N>
__device__ __forceinline__ void wave_tree_sums(float (&v)[N]) {
#pragma unroll
    for (int k = 0; k < N; k++) {
        if constexpr (T == WaveTree::DppRows) {
            v[k] = wave_sum(v[k]);
        } else {
            for (int off = 32; off >= 1; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
        }
    }
}
template <WaveTree T>
__device__ __forceinline__ float wave_tree_sum(float v) {
    float one[1] = {v};
    wave_tree_sums<T>(one);
    return one[0];
}

// Steps 2 and 3: every lane of the SET_BLOCK (workgroup blockIdx.x = part p of set b) calls it with its own sums; the
// part's STRIDE floats of partial [sets, parts, STRIDE] are stored, the entries N .. STRIDE - 1 as 0.  `staged` is the
// caller's: a kernel that walks several sets alternates two buffers, so that the next set's staging cannot overtake this
// set's reads without a second barrier.  (b and parts, not the part's address: an address formed by the caller was
// computed by every lane ahead of the tree, in vector registers.)
template <int N, WaveTree T, int STRIDE = N>
__device__ __forceinline__ void set_store_partial(float (&acc)[N], float (*staged)[N], float* __restrict__ partial, int b,
                                                  int parts) {
    static_assert(STRIDE >= N && STRIDE <= SET_BLOCK, "one lane per stored entry");
    wave_tree_sums<T>(acc);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) staged[threadIdx.x >> 6][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < STRIDE) {
        const int k = threadIdx.x;
        partial[((size_t)b * parts + blockIdx.x) * STRIDE + k] =
            k < N ? ((staged[0][k] + staged[1][k]) + staged[2][k]) + staged[3][k] : 0.0f;
    }
}

// Step 4: s = the sums of set b; part p's N sums are at partial[(b parts + p) STRIDE + k].  (No __restrict__ on partial: the
// kernels' own arguments carry it, and with it here the camera's finish waited for each load of a part before the next.)
template <int N, int STRIDE = N>
__device__ __forceinline__ void set_add_parts(const float* partial, int b, int parts, float (&s)[N]) {
#pragma unroll
    for (int k = 0; k < N; k++) s[k] = 0.0f;
    for (int p = 0; p < parts; p++) {
#pragma unroll
        for (int k = 0; k < N; k++) s[k] += partial[((size_t)b * parts + p) * STRIDE + k];
    }
}

// Where entry j of a set's row goes: column `col` of the parameter's gradient dst [batch, width] (NULL: not wanted);
// `zero`: the entry is a constant 0 and is not read from the row.
struct SetRoute {
    float* dst;
    int batch, col, width;
    bool zero;
};

// Step 5, by every lane of the finish workgroup after the barrier that follows its writes of rows [B, ROW]: route(j) for
// j < OUT (entries ROW .. OUT - 1 exist only as zeros).
template <int ROW, int OUT, class Route>
__device__ __forceinline__ void set_route_rows(const float* rows, int B, Route route) {
    for (int e = threadIdx.x; e < OUT * (B + 1); e += SET_BLOCK) {
        const int b = e / OUT, j = e % OUT;             // b == B: the sum over the sets (parameters of batch 1)
        const SetRoute r = route(j);
        if (!r.dst) continue;
        if (r.batch > 1 && b < B) {
            r.dst[(size_t)b * r.width + r.col] = r.zero ? 0.0f : rows[(size_t)b * ROW + j];
        } else if (r.batch <= 1 && b == B) {
            float t = 0.0f;
            if (!r.zero)
                for (int v = 0; v < B; v++) t += rows[(size_t)v * ROW + j];
            r.dst[r.col] = t;
        }
    }
}

}  // namespace d3m
