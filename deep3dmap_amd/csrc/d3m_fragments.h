// d3m_fragments.h -- a coverage record as the kernels read it (AttrMaps) and the walks every node that draws over one shares:
// the index expressions, the output-pixel walk of the forwards (d3m_attributes.h, d3m_uv_texture.h, d3m_uv_texture_mip.h) and
// the per-visible-face sum over owned pixels of the adjoints' stage 1 (d3m_attributes.h, d3m_fragment_geometry.h).  A node
// supplies its per-pixel arithmetic -- two callables or a policy -- and keeps its __global__ kernels; the walks are stated here once.
//
// THE ORDER of stage 1, the same bits on every run (no float atomics anywhere, nothing is cleared).  Per visible face (b, fn),
// whose clipped box (pixel_bbox, d3m_forward.h) is x0..x1 by y0..y1, bw = x1 - x0 + 1 wide, its pixels numbered row-major:
// box pixel i is (x0 + i mod bw, y0 + i div bw).  Each of the node's N accumulators is the sum of the node's per-pixel term
// over the pixels p of the box with face_index_map[b,p] == fn:
//   a. a box of at most FM_MAX_BBOX_AREA pixels: FM_LANES (8) lanes share scan_owned_pixels (d3m_face_major.h).  The box is
//      cut into chunks of 32 consecutive box pixels (the last one may be short).  WITHIN EACH CHUNK the owned pixels are
//      ranked 0, 1, ... in ascending box order and lane `sub` takes those of rank sub, sub + 8, sub + 16, sub + 24 -- the ranks
//      start again at 0 in every chunk; they do not run over the whole box.  A lane starts from +0 and adds its pixels of
//      chunk 0 in that order, then those of chunk 1, and so on.  The eight lanes a_0..a_7 are combined by quad_sum (v +=
//      lane ^ 1's, v += lane ^ 2's, v += lane (7 - l)'s) and lane 0 stores ((a_0 + a_1) + (a_2 + a_3)) + ((a_7 + a_6) + (a_5 + a_4));
//   b. a larger box: one workgroup of RG_BLOCK (256) lanes; lane t starts from +0 and adds the owned pixels among box pixels
//      t, t + 256, t + 512, ... in that order; each wave's 64 lanes are combined by the butterfly v += shfl_xor(v, off), off =
//      32, 16, ..., 1, and the result is s = 0; s += wave[w] for w = 0..3 (rg_block_sum: steps 2 and 3 of d3m_row_gather.h).
// The sums are stored plainly; entries of faces that own no pixel are never written and never read.
// tests/fragment_walk_replay.py restates both routes and tests/test_gpu_fragment_walks.py compares every word with it.
#pragma once
#include "d3m_face_major.h"
#include "d3m_row_gather.h"

namespace d3m {

constexpr int VA_CHUNK = 8;          // channels a lane keeps in registers at a time (attributes.CHANNEL_CHUNK)

// A coverage record as the kernels read it (row 0 of the maps = bottom).
struct AttrMaps {
    const int32_t* face_index_map;   // [B,S,S]
    const float* weight_map;         // [B,S,S,3]
    const float* depth_map;          // [B,S,S]
    const float* faces;              // [B,Fp,3,3] the dense copy: only owners' entries are defined, only those are read
    const int32_t* tri;              // [Ft,3]
    int B, S, Ft, Fp, aa;
};

// ---- index helpers --------------------------------------------------------------------------------------------------------
// the internal pixel of lane p: false past the batch; fn = -1 where uncovered
__device__ __forceinline__ bool fr_pixel(const AttrMaps& m, long p, int& b, int& x, int& y, int& fn) {
    const long S2 = (long)m.S * m.S;
    if (p >= (long)m.B * S2) return false;
    b = (int)(p / S2);
    const int r = (int)(p - (long)b * S2);
    y = r / m.S;
    x = r - y * m.S;
    fn = m.face_index_map[p];
    if ((unsigned)fn >= (unsigned)m.Fp) fn = -1;
    return true;
}

// the corner depths of a face's nine screen-space floats / of owner fn of view b
__device__ __forceinline__ void fr_corner_depths(const float* face, float* z) {
    z[0] = face[2];
    z[1] = face[5];
    z[2] = face[8];
}
__device__ __forceinline__ void fr_corner_depths(const AttrMaps& m, int b, int fn, float* z) {
    fr_corner_depths(m.faces + ((size_t)b * m.Fp + fn) * 9, z);
}

// side of the output image
__device__ __forceinline__ int fr_output_size(const AttrMaps& m) { return m.aa ? m.S / 2 : m.S; }

// the output pixel that internal pixel (x, y) feeds: rows reversed, 2 x 2 with anti-aliasing
__device__ __forceinline__ void fr_output_pixel(const AttrMaps& m, int x, int y, int& xo, int& yo) {
    yo = m.aa ? (m.S - 1 - y) >> 1 : m.S - 1 - y;
    xo = m.aa ? x >> 1 : x;
}

// index into the batch's maps of internal pixel j (0; with anti-aliasing 0..3 = (dy, dx) (0,0), (0,1), (1,0), (1,1) in OUTPUT
// orientation) behind output pixel (xo, yo) of view b
__device__ __forceinline__ size_t fr_internal_index(const AttrMaps& m, int b, int xo, int yo, int j) {
    const int yi = m.S - 1 - (m.aa ? 2 * yo + (j >> 1) : yo), xi = m.aa ? 2 * xo + (j & 1) : xo;
    return ((size_t)b * m.S + yi) * m.S + xi;
}

// u_c of internal pixel q (index into the batch's maps) owned by a face whose corner depths are z[0..2]
__device__ __forceinline__ void va_weights(const AttrMaps& m, size_t q, const float* z, float* u) {
    const float d = m.depth_map[q];
#pragma unroll
    for (int c = 0; c < 3; c++) u[c] = m.weight_map[3 * q + c] * (d / z[c]);
}

// scale * g[b, k0 + kk, out(x, y)] for the chunk's channels, scale = 1 or 1/4
__device__ __forceinline__ void va_pixel_grads(const AttrMaps& m, const float* __restrict__ g_view, int C, int k0, int x, int y,
                                               float* gs) {
    const int s = fr_output_size(m);
    int xo, yo;
    fr_output_pixel(m, x, y, xo, yo);
    const float scale = m.aa ? 0.25f : 1.0f;
    const float* g = g_view + ((size_t)k0 * s + yo) * s + xo;
#pragma unroll
    for (int kk = 0; kk < VA_CHUNK; kk++) gs[kk] = k0 + kk < C ? scale * g[(size_t)kk * s * s] : 0.0f;
}

// ---- the output-pixel walk of a forward -------------------------------------------------------------------------------------
// One lane per OUTPUT pixel (blockIdx.y = the view).  The 1 or 4 internal pixels behind it are gathered once, then the C
// channels are walked in chunks of VA_CHUNK (registers do not grow with C): acc = 0; acc += value or background of internal
// pixel j for j = 0..3 in that order -- a covered pixel's value is formed in full by the node before it is added --; images =
// acc * (1 or 1/4), alpha = n_cov * (1 or 1/4).  Adjacent lanes store adjacent pixels of one channel plane; every element of
// images and alpha is written.  The node supplies, as two callables over its own registers,
//   gather(int j, int b, size_t q, int fn)    internal pixel j is q (index into the batch's maps) of view b, owned by fn
//   float value(int j, int k)                 value of channel k at the covered internal pixel j
template <class Gather, class Value>
__device__ __forceinline__ void fr_output_pixel_walk(const AttrMaps& m, int C, const float* __restrict__ background,
                                                     float* __restrict__ images, float* __restrict__ alpha, Gather&& gather,
                                                     Value&& value) {
    const int s = fr_output_size(m);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= (long)s * s) return;
    const int yo = (int)(i / s), xo = (int)(i - (long)yo * s);
    const int np = m.aa ? 4 : 1;
    bool covered[4];
    float n_cov = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        covered[j] = false;
        if (j >= np) continue;
        const size_t q = fr_internal_index(m, b, xo, yo, j);
        const int fn = m.face_index_map[q];
        if ((unsigned)fn >= (unsigned)m.Fp) continue;                   // uncovered (-1)
        gather(j, b, q, fn);
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
                    acc[kk] += value(j, k);
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

// ---- stage 1 of an adjoint: the per-visible-face sums over owned pixels, N accumulators a face (THE ORDER above) -------------
// The node's Policy:
//   void setup(const float* face, int b)                     per-face values from the face's nine floats; b: its view
//   void add(int x, int y, size_t q, float* acc)             adds internal pixel (x, y), index q into the batch's maps, onto acc
//   void store(size_t gi, const float* acc) const            stores the N sums of face gi = b Fp + fn
// whether listed face gi has a box, and how many pixels it has
__device__ __forceinline__ bool fr_listed_face(const AttrMaps& m, long gi, float* face, int& x0, int& x1, int& y0, int& y1) {
#pragma unroll
    for (int k = 0; k < 9; k++) face[k] = m.faces[(size_t)gi * 9 + k];
    return pixel_bbox(face, m.S, x0, x1, y0, y1);
}

// a. FM_LANES lanes per listed face: a fixed grid of 256-lane workgroups strides over the visibility list (it has one entry
// per face at most)
template <int N, class Policy>
__device__ __forceinline__ void fr_face_sums(const AttrMaps& m, const int* __restrict__ list, const int* __restrict__ n_list,
                                             Policy& policy) {
    const int sub = threadIdx.x % FM_LANES;
    const long n_units = min((long)*n_list, (long)m.B * m.Fp);
    for (long un = (long)blockIdx.x * FM_FACES_PER_BLOCK + threadIdx.x / FM_LANES; un < n_units;
         un += (long)gridDim.x * FM_FACES_PER_BLOCK) {
        const long gi = list[un];
        if (gi < 0 || gi >= (long)m.B * m.Fp) continue;
        const int bn = (int)(gi / m.Fp), fn = (int)(gi - (long)bn * m.Fp);
        float face[9];
        int x0 = 0, x1 = 0, y0 = 0, y1 = 0;
        const bool boxed = fr_listed_face(m, gi, face, x0, x1, y0, y1);
        const int area = boxed ? (x1 - x0 + 1) * (y1 - y0 + 1) : 0;
        if (area > FM_MAX_BBOX_AREA) continue;                          // b's
        policy.setup(face, bn);
        float acc[N];
#pragma unroll
        for (int k = 0; k < N; k++) acc[k] = 0.0f;
        const size_t base = (size_t)bn * m.S * m.S;
        if (boxed)
            scan_owned_pixels<FM_LANES>(m.face_index_map + base, fn, m.S, x0, x1, y0, area, sub,
                                        [&](int x, int y) { policy.add(x, y, base + (size_t)y * m.S + x, acc); });
#pragma unroll
        for (int k = 0; k < N; k++) acc[k] = quad_sum(acc[k]);
        if (sub == 0) policy.store((size_t)gi, acc);
    }
}

// b. the listed faces whose box exceeds FM_MAX_BBOX_AREA, a workgroup of RG_BLOCK lanes per face.  A workgroup takes RG_BLOCK
// list entries at a time: lane t looks at entry first + t and notes it when it is large; the workgroup then walks the noted
// faces one after another (which workgroup meets which face does not matter: every face's sums are its own).
template <int N, class Policy>
__device__ __forceinline__ void fr_large_face_sums(const AttrMaps& m, const int* __restrict__ list,
                                                   const int* __restrict__ n_list, Policy& policy) {
    __shared__ int s_large[RG_BLOCK];
    const long n_units = min((long)*n_list, (long)m.B * m.Fp);
    const int t = threadIdx.x;
    for (long first = (long)blockIdx.x * RG_BLOCK; first < n_units; first += (long)gridDim.x * RG_BLOCK) {
        int mine = -1;
        if (first + t < n_units) {
            const long gi = list[first + t];
            if (gi >= 0 && gi < (long)m.B * m.Fp) {
                float face[9];
                int x0, x1, y0, y1;
                if (fr_listed_face(m, gi, face, x0, x1, y0, y1) && (x1 - x0 + 1) * (y1 - y0 + 1) > FM_MAX_BBOX_AREA)
                    mine = (int)gi;
            }
        }
        s_large[t] = mine;
        __syncthreads();
        for (int j = 0; j < RG_BLOCK; j++) {
            const int gi = s_large[j];                                  // (the same for every lane)
            if (gi < 0) continue;
            const int bn = gi / m.Fp, fn = gi - bn * m.Fp;
            float face[9];
            int x0, x1, y0, y1;
            fr_listed_face(m, gi, face, x0, x1, y0, y1);
            const int bw = x1 - x0 + 1, area = bw * (y1 - y0 + 1);
            const size_t base = (size_t)bn * m.S * m.S;
            policy.setup(face, bn);
            float acc[N];
#pragma unroll
            for (int k = 0; k < N; k++) acc[k] = 0.0f;
            for (int i = t; i < area; i += RG_BLOCK) {
                const int by = i / bw, x = x0 + (i - by * bw), y = y0 + by;
                const size_t q = base + (size_t)y * m.S + x;
                if (m.face_index_map[q] != fn) continue;
                policy.add(x, y, q, acc);
            }
            rg_block_sum(acc);                                          // steps 2 and 3 of d3m_row_gather.h
            if (t == 0) policy.store((size_t)gi, acc);
            __syncthreads();                                            // (rg_block_sum's staging array is used again)
        }
        __syncthreads();
    }
}

}  // namespace d3m
