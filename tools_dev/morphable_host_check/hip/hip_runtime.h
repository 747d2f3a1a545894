// A stand-in for <hip/hip_runtime.h> that lets csrc/d3m_morphable.h compile for the host: a workgroup is blockDim.x threads
// and a barrier, __shared__ is static storage (one workgroup runs at a time), launch() walks the grid.
#pragma once
#include <algorithm>
#include <barrier>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <thread>
#include <vector>
struct dim3 {
    unsigned x, y, z;
    dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
struct alignas(16) float4 { float x, y, z, w; };
inline float4 make_float4(float a, float b, float c, float d) { return {a, b, c, d}; }
inline thread_local dim3 threadIdx, blockIdx;
inline dim3 gridDim, blockDim;
inline std::barrier<>* g_barrier = nullptr;
inline void __syncthreads() { g_barrier->arrive_and_wait(); }
#define __global__
#define __shared__ static
#define __launch_bounds__(n)
#define __restrict__
using std::min;
template <class F>
void launch(dim3 grid, dim3 block, F kernel) {
    gridDim = grid;
    blockDim = block;
    std::barrier<> bar(block.x);
    g_barrier = &bar;
    std::vector<std::thread> threads;
    for (unsigned t = 0; t < block.x; t++)
        threads.emplace_back([=, &bar] {
            threadIdx = dim3(t);
            for (unsigned bz = 0; bz < grid.z; bz++)
                for (unsigned by = 0; by < grid.y; by++)
                    for (unsigned bx = 0; bx < grid.x; bx++) {
                        blockIdx = dim3(bx, by, bz);
                        kernel();
                        bar.arrive_and_wait();      // the next workgroup reuses the static storage
                    }
        });
    for (auto& th : threads) th.join();
}
