// d3m_row_gather.h -- the long-row format of a gathered CSR and its fixed summation tree, stated once for every node that
// gathers over a CSR (d3m_textures.h: the uv transpose; d3m_vertex_colors.h and d3m_smooth_shade.h: the faces' adjacency;
// d3m_mesh_reg.h: the neighbour and the wing CSR).  The ABI's d3m_csr (include/d3m_raster.h) carries it, CsrRows below is its
// device side, and neural_renderer/row_gather.py builds it.
//
// A row of up to long_row items is summed by its own lane(s) in item order (how many lanes is the node's business).  A
// longer row (a hub: pixel (0,0) of a uv layout, a fan apex, a pole) must not make one lane walk thousands of items: it is
// listed in long_rows (ascending) and cut into chunks [start, end) of the item array, row l owning the chunks
// long_chunk_ptr[l] .. long_chunk_ptr[l + 1].  THE ORDER of a long row's sum, the same bits on every run:
//   1. one workgroup of RG_BLOCK lanes per chunk; lane t adds the terms of items start + t, start + t + RG_BLOCK, ... in
//      that order, from 0;
//   2. the 64 lanes of a wave are combined by the butterfly v += __shfl_xor(v, off, 64), off = 32, 16, ..., 1
//      (d3m_set_sums.h's WaveTree::XorButterfly; its DppRows is another tree and is not used here);
//   3. lane 0 of each wave stages its sum; after one barrier the chunk's sum is s = 0; s += wave[w] for w = 0 .. 3
//      (from 0: not the combine of d3m_set_sums.h, which starts from wave 0's value);
//   4. the row adds its chunks' sums in chunk order, onto whatever it holds already.
// No float atomics, and no workgroup waits for another: the chunk sums go through a partials array between two launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "d3m_set_sums.h"

namespace d3m {

constexpr int RG_BLOCK = 256;

// One CSR's long-row tables.
struct LongRows {
    const int2* chunks;              // [n_chunks] item ranges [start, end)
    const int32_t* rows;             // [n_rows] the long rows, ascending
    const int32_t* chunk_ptr;        // [n_rows + 1] row l owns chunks chunk_ptr[l] .. chunk_ptr[l + 1]
    int n_chunks, n_rows, long_row;
};

// A gathered CSR as a kernel receives it: the device side of d3m_csr (include/d3m_raster.h), made by the host's csr_rows().
struct CsrRows {
    const int32_t* offsets;          // [rows + 1]
    const int32_t* items;            // the node's item layout
    LongRows longs;
};

// whether a row of n_items items went through the chunks
__device__ __forceinline__ bool rg_is_long(const LongRows& t, int n_items) { return n_items > t.long_row && t.n_rows > 0; }

// index of the long row `v` in t.rows (which holds v): the first index whose entry is >= v
__device__ __forceinline__ int rg_find_long(const LongRows& t, int v) {
    int lo = 0, hi = t.n_rows - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t.rows[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the long row that owns chunk `ch`: the last l with chunk_ptr[l] <= ch
__device__ __forceinline__ int rg_chunk_owner(const LongRows& t, int ch) {
    int lo = 0, hi = t.n_rows - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (t.chunk_ptr[mid] <= ch) lo = mid; else hi = mid - 1;
    }
    return t.rows[lo];
}

// Steps 2 and 3 for N components: v becomes the workgroup's sum in every lane.  Every lane of the RG_BLOCK calls it, once
// per kernel and N (the staging array is not guarded for a second use).
template <int N>
__device__ __forceinline__ void rg_block_sum(float (&v)[N]) {
    __shared__ float staged[RG_BLOCK / 64][N];
    wave_tree_sums<WaveTree::XorButterfly>(v);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) staged[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < RG_BLOCK / 64; w++) s += staged[w][k];
        v[k] = s;
    }
}

// Step 1: term(e, acc) adds item e's term onto this lane's acc.
template <int N, class Term>
__device__ __forceinline__ void rg_lane_sum(int2 range, float (&acc)[N], Term term) {
    for (int e = range.x + (int)threadIdx.x; e < range.y; e += RG_BLOCK) term(e, acc);
}

// Steps 1 to 3: the sum of one chunk, in every lane.
template <int N, class Term>
__device__ __forceinline__ void rg_chunk_sum(int2 range, float (&sum)[N], Term term) {
#pragma unroll
    for (int k = 0; k < N; k++) sum[k] = 0.f;
    rg_lane_sum(range, sum, term);
    rg_block_sum(sum);
}

// Step 4: adds the chunk sums of long row l onto acc; chunk c's N sums are at part[c * STRIDE + k].
template <int N, int STRIDE = N>
__device__ __forceinline__ void rg_add_chunk_sums(const LongRows& t, int l, const float* __restrict__ part, float (&acc)[N]) {
    for (int c = t.chunk_ptr[l]; c < t.chunk_ptr[l + 1]; c++) {
#pragma unroll
        for (int k = 0; k < N; k++) acc[k] += part[(size_t)c * STRIDE + k];
    }
}

}  // namespace d3m
