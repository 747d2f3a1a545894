// A stand-in for csrc/d3m_aux.h that lets csrc/d3m_pose.h compile for the host on ../morphable_host_check's workgroup shim:
// the two 3x3 helpers are cut out of the real header by run.sh (aux_helpers.inc), wave_sum is the tree of csrc/d3m_device.h
// (quad swaps, the two mirrors of a 16-lane row, then (r0 + r1) + (r2 + r3)) over a snapshot of the workgroup's values.
#pragma once
#include <hip/hip_runtime.h>
#define __device__
#define __host__
#define __forceinline__ inline
namespace d3m {
#include "aux_helpers.inc"
inline float wave_sum(float v) {
    static float snap[1024];
    snap[threadIdx.x] = v;
    __syncthreads();
    const float* w = snap + (threadIdx.x & ~63u);
    float r[4];
    for (int row = 0; row < 4; row++) {
        float a[16], b[16], c[16];
        for (int i = 0; i < 16; i++) a[i] = w[16 * row + i] + w[16 * row + (i ^ 1)];
        for (int i = 0; i < 16; i++) b[i] = a[i] + a[i ^ 2];
        for (int i = 0; i < 16; i++) c[i] = b[i] + b[(i & ~7) + 7 - (i & 7)];
        r[row] = c[0] + c[15];
    }
    __syncthreads();            // the snapshot is free again
    return (r[0] + r[1]) + (r[2] + r[3]);
}
}  // namespace d3m
