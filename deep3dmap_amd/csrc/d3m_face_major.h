// d3m_face_major.h -- atomic-free forms of the texture and depth backward passes.
//
// The reference scatters from pixels with float atomics: 24 per covered pixel for the texture cube
// (KCU:531-538), 9 for the depth gradient (KCU:573-590).  A face owns only the pixels inside its
// bounding box, so the sums can instead be GATHERED: FM_LANES lanes per visible face share the walk over its
// (small) bounding box -- owner indices over the whole box, everything else for the pixels the face owns
// (scan_owned_pixels) --, keep the sums in registers / LDS, combine them and store once.  Faces that own no pixel
// (culled, hidden or off screen: ~95% of the 2F' faces of a closed mesh) are skipped via a visibility
// flag; faces with a large bounding box fall back to the per-pixel atomic kernels.
#pragma once
#include <type_traits>
#include "d3m_backward.h"
#include "d3m_forward.h"

namespace d3m {

#ifndef D3M_FM_MAX_BBOX_AREA
#define D3M_FM_MAX_BBOX_AREA 4096
#endif
constexpr int FM_MAX_BBOX_AREA = D3M_FM_MAX_BBOX_AREA;   // larger faces are left to the per-pixel atomic kernels
// Lanes per face.  The bounding-box scan is a chain of dependent loads (owner index, then the pixel's maps): one
// lane per face serialises ~10-25 of them.  FM_LANES adjacent lanes share a face, take every FM_LANES-th pixel of
// its box and combine their partial sums with quad shuffles / LDS; the visible faces of a mesh come in long index
// runs, so the waves stay dense.
constexpr int FM_LANES = 8;
constexpr int FM_FACES_PER_BLOCK = 256 / FM_LANES;

// ---- the owned-pixel scan: every gathered pass walks a face's box through this one helper ------------------------------
// A face owns about a quarter of the pixels of its box (headline scene: 7.0 of 28.3), so a scan that loads a pixel's maps
// and runs its arithmetic for every box pixel spends three quarters of both on contributions that are selected to zero.
// scan_owned_pixels() takes the box in chunks of LANES * K consecutive box pixels (row-major: pixel i is column i % width,
// row i / width of the box):
//   A. every lane requests the K owner indices at chunk offsets sub, sub + LANES, ... together (4 B a pixel, one round
//      trip a chunk) and nothing else; ballot(owner == fn) of offset k hands each group of LANES lanes its LANES bits, and
//      the K of them form the group's mask M: bit j = "the face owns the chunk's pixel j";
//   B. the owned pixels are numbered in ascending box order and lane `sub` takes those of rank sub, sub + LANES, ... --
//      the position of the n-th set bit of M -- and calls body(x, y) for them only.
// The pixel set is exactly {p in box : face_index_map[p] == fn} and the order in which a lane meets its pixels (hence the
// order of every sum the bodies keep) is a function of the maps alone, the same for every kernel that scans through here.
// The next chunk's A is requested before the current chunk's B, so that its round trip overlaps the dense steps.
// No LDS, no cross-lane traffic but the ballots.  The lanes of a group stay together through A; the groups of a wave run
// as many chunks as their own box has (a ballot then sees the finished groups' bits as 0, and a group reads only its own).

// position of the n-th (0-based) set bit of m; n < popcount(m)
__device__ __forceinline__ int nth_set_bit(uint32_t m, int n) {
    int pos = 0, c = __popc(m & 0xFFFFu);
    if (n >= c) { n -= c; pos = 16; m >>= 16; }
    c = __popc(m & 0xFFu);
    if (n >= c) { n -= c; pos += 8; m >>= 8; }
    c = __popc(m & 0xFu);
    if (n >= c) { n -= c; pos += 4; m >>= 4; }
    c = __popc(m & 0x3u);
    if (n >= c) { n -= c; pos += 2; m >>= 2; }
    if (n >= (int)(m & 1u)) pos += 1;
    return pos;
}
__device__ __forceinline__ int nth_set_bit(uint64_t m, int n) {
    const uint32_t lo = (uint32_t)m, hi = (uint32_t)(m >> 32);
    const int c = __popc(lo);
    return n >= c ? 32 + nth_set_bit(hi, n - c) : nth_set_bit(lo, n);
}

// t = q * bw + r, 0 <= r < bw, for 0 <= t < bw + 64 and bw < 2^22: both floats are exact, the reciprocal is within 1 ulp
// and q < 66, so the truncated product is q or a neighbour -- one step either way repairs it (an integer division is ~30
// instructions)
__device__ __forceinline__ void box_split(int t, int bw, float rbw, int& q, int& r) {
    q = (int)((float)t * rbw);
    r = t - q * bw;
    if (r < 0) { q--; r += bw; }
    if (r >= bw) { q++; r -= bw; }
}

// fim_view: the view's face_index_map; the box is x0..x1 by y0.. with `area` pixels; sub: this lane among the LANES of its
// face, which are adjacent lanes of one wave starting at a multiple of LANES (blocks are 1-D)
template <int LANES, class Body>
__device__ __forceinline__ void scan_owned_pixels(const int32_t* __restrict__ fim_view, int fn, int S, int x0, int x1, int y0,
                                                  int area, int sub, Body&& body) {
    static_assert(LANES == 64 || (LANES <= 16 && 32 % LANES == 0), "a chunk is one 32-bit mask per group, or the wave's ballot");
    constexpr int K = LANES == 64 ? 1 : 32 / LANES, CHUNK = LANES * K;
    const int bw = x1 - x0 + 1;
    const float rbw = __builtin_amdgcn_rcpf((float)bw);
    const int shift = (int)(threadIdx.x & 63u) - sub;      // the group's first lane in the wave
    int cr = 0, cy = y0;                                   // the chunk's first pixel: column within the box, row
    // A: owners only
    auto request_owners = [&](int cb, int cr_, int cy_, int32_t* owner) {
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int o = k * LANES + sub;
            int q, r;
            box_split(cr_ + o, bw, rbw, q, r);
            owner[k] = cb + o < area ? fim_view[(size_t)(cy_ + q) * S + (x0 + r)] : -1;    // (past the box: no load, never fn)
        }
    };
    int32_t owner[K];
    request_owners(0, cr, cy, owner);
    for (int cb = 0; cb < area; cb += CHUNK) {
        typename std::conditional<LANES == 64, uint64_t, uint32_t>::type m;
        if constexpr (LANES == 64) {
            m = __builtin_amdgcn_ballot_w64(owner[0] == fn);
        } else {
            m = 0;
#pragma unroll
            for (int k = 0; k < K; k++) {
                const uint64_t bal = __builtin_amdgcn_ballot_w64(owner[k] == fn);
                m |= ((uint32_t)(bal >> shift) & ((1u << LANES) - 1u)) << (k * LANES);
            }
        }
        // the next chunk's owners are requested before this chunk's pixels: their round trip overlaps the dense steps
        int nq, nr;
        box_split(cr + CHUNK, bw, rbw, nq, nr);
        if (cb + CHUNK < area) request_owners(cb + CHUNK, nr, cy + nq, owner);
        // B: dense
        const int cnt = LANES == 64 ? __popcll(m) : __popc((uint32_t)m);
        for (int n = sub; n < cnt; n += LANES) {           // (a wave per face: at most one step)
            int q, r;
            box_split(cr + nth_set_bit(m, n), bw, rbw, q, r);
            body(x0 + r, cy + q);
        }
        cy += nq;
        cr = nr;
    }
}

// sum over the FM_LANES (= 8) adjacent lanes of a face, in every one of them: two quad swaps and the half-row
// mirror, all DPP (no LDS crossbar)
__device__ __forceinline__ float quad_sum(float v) {
    static_assert(FM_LANES == 8, "quad_sum is written for 8 lanes per face");
    v += dpp_f32<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_f32<0x4E>(v);      // quad_perm [2,3,0,1]
    v += dpp_f32<0x141>(v);     // row_half_mirror: the other quad of the 8
    return v;
}
constexpr int FLAG_HIDDEN = 0, FLAG_VISIBLE = 1, FLAG_LARGE = 2;

// flags[b*F + f] = 1 for every face that owns at least one pixel (plain stores of the same value)
__global__ void __launch_bounds__(256) k_mark_visible(const int32_t* __restrict__ face_index_map, int* __restrict__ flags,
                                                     int B, int F, int S) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * S * S) return;
    const int fi = face_index_map[i];
    if (fi >= 0) flags[(size_t)(i / ((long)S * S)) * F + fi] = FLAG_VISIBLE;
}

// Depth backward, gathered: KCU:543-592 summed over the pixels a face owns.  The sums go to grad_faces (+=) or, with a
// vertex target, straight into the gradient of the vertices the faces were gathered from (float atomics).
// LANES adjacent lanes share a face: FM_LANES (8) for ordinary meshes, a whole wave (64) for coarse ones, whose faces of
// hundreds of pixels were ninety steps of dependent loads for each of eight lanes (722 triangles @512^2: 234 us).
template <class FS, int LANES>
__device__ __forceinline__ void backward_depth_face(FS fs, const float* __restrict__ depth_map,
                                                    const int32_t* __restrict__ face_index_map,
                                                    const float* __restrict__ weight_map,
                                                    const float* __restrict__ grad_depth_map, float* __restrict__ grad_faces,
                                                    int* __restrict__ flags, int S, long gi, int sub, int F,
                                                    const VertexTarget& vt, int* __restrict__ n_large, int flip_rows,
                                                    int max_area) {
    const int bn = (int)(gi / F), fn = (int)(gi % F);
    float face[9], finv[9];
    fs.load(bn, fn, face);
    int x0, x1, y0, y1;
    if (!pixel_bbox(face, S, x0, x1, y0, y1)) return;
    const int area = (x1 - x0 + 1) * (y1 - y0 + 1);
    if (area > max_area) {      // (FM_MAX_BBOX_AREA; INT_MAX in the deterministic mode: a face's lanes own its sums whatever its size)                      // left to the per-pixel pass (counted, so that it can leave at once)
        flags[gi] = FLAG_LARGE;
        if (n_large && sub == 0) atomicAdd(n_large, 1);
        return;
    }
    face_inverse(face, S, finv);
    float tmp[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int l = 0; l < 3; l++) tmp[k] += -finv[3 * l + k] / face[3 * l + 2];     // KCU:582
    }
    float acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const size_t base = (size_t)bn * S * S;
    // the pixels the face owns, and only those (scan_owned_pixels): their maps are requested together
    scan_owned_pixels<LANES>(face_index_map + base, fn, S, x0, x1, y0, area, sub, [&](int x, int y) {
        const size_t p = base + (size_t)y * S + x;
        // (flip_rows: the gradient is that of the OUTPUT image, whose row S-1-y is the map's row y -- rasterize.py:311-317)
        const float depth = depth_map[p], g = grad_depth_map[flip_rows ? base + (size_t)(S - 1 - y) * S + x : p];
        const float lw[3] = {weight_map[3 * p], weight_map[3 * p + 1], weight_map[3 * p + 2]};
        const float depth2 = depth * depth;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float wk = lw[k], z_k = face[3 * k + 2];
            acc[3 * k + 0] += -g * tmp[0] * wk * depth2 * (float)S / 2.0f;          // KCU:588
            acc[3 * k + 1] += -g * tmp[1] * wk * depth2 * (float)S / 2.0f;
            acc[3 * k + 2] += g * wk * depth2 / (z_k * z_k);                        // KCU:575
        }
    });
#pragma unroll
    for (int k = 0; k < 9; k++) acc[k] = LANES == 64 ? wave_sum(acc[k]) : quad_sum(acc[k]);
    if (sub == 0) {
        if (vt.gv) {
#pragma unroll
            for (int v = 0; v < 3; v++) {
                float* g = vt.vertex(bn, fn, v);
#pragma unroll
                for (int k = 0; k < 3; k++) atomicAdd(&g[k], acc[3 * v + k]);
            }
        } else {
            float* gf = grad_faces + (size_t)gi * 9;
#pragma unroll
            for (int k = 0; k < 9; k++) gf[k] += acc[k];
        }
    }
}

// Over every face of the batch (flags decide), or -- `list`, the compacted list of d3m_visibility -- over the faces that own
// a pixel: a fixed grid striding either way (the FM_LANES lanes of a face stay together).
template <class FS, int LANES = FM_LANES>
__global__ void __launch_bounds__(256) k_backward_depth_faces(FS fs, const float* __restrict__ depth_map,
                                                             const int32_t* __restrict__ face_index_map,
                                                             const float* __restrict__ weight_map,
                                                             const float* __restrict__ grad_depth_map,
                                                             float* __restrict__ grad_faces, int* __restrict__ flags, int B,
                                                             int S, const int* __restrict__ list,
                                                             const int* __restrict__ n_list, VertexTarget vt,
                                                             int* __restrict__ n_large, int flip_rows, int max_area) {
    static_assert(LANES == FM_LANES || LANES == 64, "eight lanes per face, or a wave");
    const int sub = threadIdx.x % LANES;
    const int F = fs.num_faces();
    const long n_units = list ? (long)*n_list : (long)B * F;
    for (long u = (long)blockIdx.x * (256 / LANES) + threadIdx.x / LANES; u < n_units; u += (long)gridDim.x * (256 / LANES)) {
        const long gi = list ? (long)list[u] : u;
        if (!list && flags[gi] == FLAG_HIDDEN) continue;
        backward_depth_face<FS, LANES>(fs, depth_map, face_index_map, weight_map, grad_depth_map, grad_faces, flags, S, gi, sub, F, vt,
                            n_large, flip_rows, max_area);
    }
}

// Texture backward for ts == 2, gathered: 8 texels x 3 channels per face kept in LDS.  grad_textures += .
template <class FS>
__global__ void __launch_bounds__(256) k_backward_textures_faces(FS fs, const int32_t* __restrict__ face_index_map,
                                                                const float* __restrict__ sampling_weight_map,
                                                                const int32_t* __restrict__ sampling_index_map,
                                                                const float* __restrict__ grad_rgb_map,
                                                                float* __restrict__ grad_textures, int* __restrict__ flags,
                                                                int B, int S) {
    __shared__ float s_acc[24][256];
    const long gi = (long)blockIdx.x * FM_FACES_PER_BLOCK + threadIdx.x / FM_LANES;
    const int sub = threadIdx.x % FM_LANES;
    const int F = fs.num_faces();
    if (gi >= (long)B * F || flags[gi] == FLAG_HIDDEN) return;
    const int bn = (int)(gi / F), fn = (int)(gi % F);
    float face[9];
    fs.load(bn, fn, face);
    int x0, x1, y0, y1;
    if (!pixel_bbox(face, S, x0, x1, y0, y1)) return;
    const int area = (x1 - x0 + 1) * (y1 - y0 + 1);
    if (area > FM_MAX_BBOX_AREA) { flags[gi] = FLAG_LARGE; return; }
    const int l = threadIdx.x;
#pragma unroll
    for (int t = 0; t < 24; t++) s_acc[t][l] = 0;
    const size_t base = (size_t)bn * S * S;
    scan_owned_pixels<FM_LANES>(face_index_map + base, fn, S, x0, x1, y0, area, sub, [&](int x, int y) {
        const size_t p = base + (size_t)y * S + x;
        const float g0 = grad_rgb_map[3 * p + 0], g1 = grad_rgb_map[3 * p + 1], g2 = grad_rgb_map[3 * p + 2];
#pragma unroll
        for (int pn = 0; pn < 8; pn++) {
            const float w = sampling_weight_map[p * 8 + pn];
            const int isc = sampling_index_map[p * 8 + pn] & 7;                     // ts == 2: 0..7
            s_acc[isc * 3 + 0][l] += w * g0;                                        // KCU:537
            s_acc[isc * 3 + 1][l] += w * g1;
            s_acc[isc * 3 + 2][l] += w * g2;
        }
    });
    // the face's lanes sit in one wave: their LDS columns are complete once the loop has reconverged
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (sub == 0) {
        float* gt = grad_textures + (size_t)gi * 24;
#pragma unroll
        for (int t = 0; t < 24; t++) {
            float v = s_acc[t][l];
#pragma unroll
            for (int j = 1; j < FM_LANES; j++) v += s_acc[t][l + j];
            gt[t] += v;
        }
    }
}

}  // namespace d3m
