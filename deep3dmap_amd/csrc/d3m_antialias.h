// d3m_antialias.h -- analytic edge antialiasing of an image drawn over a coverage record (AttrMaps, d3m_fragments.h), and its
// adjoint with respect to the image and to the screen-space vertices: the SILHOUETTE gradient of the coverage-record family.
// The two pixels on either side of a silhouette edge are blended by how far the edge sits between their centres, so image
// values near the outline are continuous functions of the vertex positions.  Records without anti-aliasing only (S = s).
//
// The function, in the maps' orientation (internal pixel (x, y) = output pixel (x, S - 1 - y); centre P = (pixel_center(x),
// pixel_center(y))).  tid(p) = face_index_map[b,p] mod Ft (-1: uncovered), c(p) = the image's C values at p.  For every
// unordered pair of 4-neighbours p, q = p + (1,0) or p + (0,1) inside the image (aa_pair, the ONE decision all kernels call):
//   1. tid(p) == tid(q): nothing.
//   2. n = the covered pixel with the smaller depth_map value (uncovered = +inf; a tie: p), o the other; T = the owner of n,
//      corners (X_k, Y_k) = faces[b,fn]; w = the sign of den = (X1 - X0)(Y2 - Y0) - (X2 - X0)(Y1 - Y0).
//   3. the exit edge (aa_exit_edge): side k runs from corner a = k to c = (k + 1) mod 3, E_k(P) = (X_c - X_a)(P_y - Y_a) -
//      (Y_c - Y_a)(P_x - X_a).  Side k qualifies when E_k(P_n) w >= 0 and E_k(P_o) w < 0; t_k = E_k(P_n) / D_k with D_k =
//      E_k(P_n) - E_k(P_o) in closed form (P_o - P_n is one pixel step along one axis: D_k = (Y_c - Y_a) step for a horizontal
//      pair, -(X_c - X_a) step for a vertical one -- no subtraction of nearly equal numbers).  The edge is the qualifying side
//      of smallest t, the lowest k on a tie; no qualifying side (o lies inside T but belongs to a nearer surface: an
//      intersection): nothing.
//   4. j = the side in the underlying triangle (k, or (1 - k) mod 3 for a fill_back copy); opp = side_opposite[f,j]
//      (neural_renderer/antialias.py builds it): -1 a boundary (a silhouette), -2 nothing, else the third vertex O of the one
//      other triangle on the edge: a silhouette iff E_k(O) w >= 0 (the neighbour folds back onto T's side), else nothing.
//   5. t = t_k.  t > 1/2: out(o) += (t - 1/2)(c(n) - c(o));  t < 1/2: out(n) += (1/2 - t)(c(o) - c(n));  t = 1/2: nothing.
// out starts as c; a pixel adds the pairs in which it is the recipient in the slot order -x, +x, -y, +y.  The choices of near
// pixel, edge and recipient are NOT differentiated; t is.
//
// Kernels (256 lanes, one lane per internal pixel, channels in chunks of VA_CHUNK; no float atomics, nothing cleared, every
// output element written):
//   k_antialias_images           out(r) as above: each pair is evaluated by both of its pixels (a gather).
//   k_antialias_images_backward  g_in(r) = g_out(r); then per slot, with recipient m, donor d, weight |t - 1/2|:  -= weight
//                                g_out(r) when r = m, += weight g_out(m) when r = d.  And pair_grads[b,r,slot] = dL/dt = sum
//                                over channels k ascending from 0 of g_out(m)[k] (c(n)[k] - c(o)[k]) when r is the pair's near
//                                pixel, +0 otherwise: a [B,S,S,4] map.
//   stage 1 of the vertex adjoint (AaFaceSums over fr_face_sums<9> / fr_large_face_sums<9>, THE ORDER of d3m_fragments.h):
//     per visible face, over the pixels it owns, for slot -x, +x, -y, +y with g = pair_grads != 0: the exit edge again from
//     T's corners, N = E(P_n), Eo = E(P_o), D as above; gN = -g Eo / D^2, gE = g N / D^2; onto the accumulators of corner a:
//     x += gN (Y_c - Pn_y) + gE (Y_c - Po_y), y += gN (Pn_x - X_c) + gE (Po_x - X_c); of corner c: x += gN (Pn_y - Y_a) + gE
//     (Po_y - Y_a), y += gN (X_a - Pn_x) + gE (X_a - Po_x).  The z accumulators and the third corner stay +0.  Gv [B,F',3,3].
//   stage 2: the rows / chunks kernels of the attribute adjoint with C = 3 (face_sums_gather in d3m_raster.hip).
#pragma once
#include "d3m_fragments.h"

namespace d3m {

constexpr int AA_NONE = 0, AA_TO_FAR = 1, AA_TO_NEAR = 2;      // what a pair does: nothing, blends into o, blends into n

// what the pair decision reads beside the record
struct AaScene {
    const float* screen_vertices;    // [B,V,3]
    const int32_t* side_opposite;    // [Ft,3]
    int V;
};

// the exit edge of a triangle between two neighbouring pixel centres
struct AaEdge {
    int k;                           // the side, -1: none qualifies
    float N, Eo, D;                  // E_k(P_n), E_k(P_o), their difference in closed form
    float ax, ay, cx, cy, ex, ey;    // corners a and c, and the side's vector (X_c - X_a, Y_c - Y_a)
};

__device__ __forceinline__ float aa_face_sign(const float* face) {
    const float den = (face[3] - face[0]) * (face[7] - face[1]) - (face[6] - face[0]) * (face[4] - face[1]);
    return den > 0.0f ? 1.0f : (den < 0.0f ? -1.0f : 0.0f);
}

// step 3: near pixel (xn, yn), other pixel (xo, yo) = one step along one axis
__device__ __forceinline__ AaEdge aa_exit_edge(const float* face, float w, int xn, int yn, int xo, int yo, int S) {
    const float X[3] = {face[0], face[3], face[6]}, Y[3] = {face[1], face[4], face[7]};
    const float pnx = pixel_center(xn, S), pny = pixel_center(yn, S), pox = pixel_center(xo, S), poy = pixel_center(yo, S);
    const bool horizontal = yn == yo;
    const float step = (float)(2 * (horizontal ? xo - xn : yo - yn)) / (float)S;
    float best = 0.0f;
    int bk = -1;
    float bN = 0.0f, bEo = 0.0f, bD = 0.0f, bax = 0.0f, bay = 0.0f, bcx = 0.0f, bcy = 0.0f, bex = 0.0f, bey = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int c = (k + 1) % 3;
        const float ex = X[c] - X[k], ey = Y[c] - Y[k];
        const float N = ex * (pny - Y[k]) - ey * (pnx - X[k]);
        const float Eo = ex * (poy - Y[k]) - ey * (pox - X[k]);
        if (!(N * w >= 0.0f && Eo * w < 0.0f)) continue;
        const float D = horizontal ? ey * step : -ex * step;
        const float t = N / D;
        if (bk < 0 || t < best) {
            best = t;
            bk = k;
            bN = N; bEo = Eo; bD = D;
            bax = X[k]; bay = Y[k]; bcx = X[c]; bcy = Y[c]; bex = ex; bey = ey;
        }
    }
    return AaEdge{bk, bN, bEo, bD, bax, bay, bcx, bcy, bex, bey};
}

// steps 1 to 5 for the pair p = (xp, yp), q = p + (1,0) (axis 0) or p + (0,1) (axis 1) of view b, both inside the image:
// what the pair does, whether p is its near pixel, and t
__device__ __forceinline__ int aa_pair(const AttrMaps& m, const AaScene& sc, int b, int xp, int yp, int axis, bool& p_near,
                                       float& t) {
    const int S = m.S;
    const size_t ip = ((size_t)b * S + yp) * S + xp, iq = ip + (axis ? S : 1);
    int fp = m.face_index_map[ip], fq = m.face_index_map[iq];
    if ((unsigned)fp >= (unsigned)m.Fp) fp = -1;
    if ((unsigned)fq >= (unsigned)m.Fp) fq = -1;
    p_near = true;
    t = 0.5f;
    const int tp = fp >= m.Ft ? fp - m.Ft : fp, tq = fq >= m.Ft ? fq - m.Ft : fq;
    if (tp == tq) return AA_NONE;
    const float dp = fp >= 0 ? m.depth_map[ip] : INFINITY, dq = fq >= 0 ? m.depth_map[iq] : INFINITY;
    p_near = fq < 0 || (fp >= 0 && dp <= dq);
    const int fn = p_near ? fp : fq;
    const int xq = xp + (axis ? 0 : 1), yq = yp + (axis ? 1 : 0);
    float face[9];
    const float* src = m.faces + ((size_t)b * m.Fp + fn) * 9;
#pragma unroll
    for (int k = 0; k < 9; k++) face[k] = src[k];
    const float w = aa_face_sign(face);
    const AaEdge e = aa_exit_edge(face, w, p_near ? xp : xq, p_near ? yp : yq, p_near ? xq : xp, p_near ? yq : yp, S);
    if (e.k < 0) return AA_NONE;
    const bool back = fn >= m.Ft;
    const int j = back ? (4 - e.k) % 3 : e.k;
    const int opp = sc.side_opposite[(size_t)(back ? fn - m.Ft : fn) * 3 + j];
    if (opp < -1 || opp >= sc.V) return AA_NONE;
    if (opp >= 0) {
        const float* O = sc.screen_vertices + ((size_t)b * sc.V + opp) * 3;
        const float EO = e.ex * (O[1] - e.ay) - e.ey * (O[0] - e.ax);
        if (!(EO * w >= 0.0f)) return AA_NONE;                            // an interior edge
    }
    t = e.N / e.D;
    return t > 0.5f ? AA_TO_FAR : (t < 0.5f ? AA_TO_NEAR : AA_NONE);
}

// One of pixel r's four pairs, slot 0..3 = -x, +x, -y, +y, as r sees it.
constexpr int AA_IDLE = 0, AA_RECIPIENT = 1, AA_DONOR = 2;
struct AaSlot {
    int role;                        // of r in the pair
    bool near;                       // r is the pair's near pixel (only meaningful when role != AA_IDLE)
    float weight;                    // |t - 1/2|
    size_t other;                    // the other pixel's offset inside one channel plane of the OUTPUT-oriented image
};

__device__ __forceinline__ void aa_slot(const AttrMaps& m, const AaScene& sc, int b, int x, int y, int slot, AaSlot& s) {
    const int S = m.S;
    const int axis = slot >> 1, up = slot & 1;                            // up: r is the pair's p
    const int xo = x + (axis ? 0 : (up ? 1 : -1)), yo = y + (axis ? (up ? 1 : -1) : 0);
    s.role = AA_IDLE;
    s.near = false;
    s.weight = 0.0f;
    s.other = 0;
    if (xo < 0 || xo >= S || yo < 0 || yo >= S) return;
    bool p_near;
    float t;
    const int act = aa_pair(m, sc, b, up ? x : xo, up ? y : yo, axis, p_near, t);
    if (act == AA_NONE) return;
    s.near = p_near == (up != 0);
    s.role = (act == AA_TO_NEAR) == s.near ? AA_RECIPIENT : AA_DONOR;
    s.weight = fabsf(t - 0.5f);
    s.other = (size_t)(S - 1 - yo) * S + xo;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_antialias_images(AttrMaps m, AaScene sc, const float* __restrict__ images, int C,
                                                          float* __restrict__ out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    int b, x, y, fn;
    if (!fr_pixel(m, p, b, x, y, fn)) return;
    const int S = m.S;
    const size_t plane = (size_t)S * S, own = (size_t)(S - 1 - y) * S + x;
    AaSlot s[4];
#pragma unroll
    for (int j = 0; j < 4; j++) aa_slot(m, sc, b, x, y, j, s[j]);
    const float* img = images + (size_t)b * C * plane;
    float* dst = out + (size_t)b * C * plane + own;
    for (int k0 = 0; k0 < C; k0 += VA_CHUNK) {
        float cr[VA_CHUNK], acc[VA_CHUNK];
#pragma unroll
        for (int kk = 0; kk < VA_CHUNK; kk++) acc[kk] = cr[kk] = k0 + kk < C ? img[(size_t)(k0 + kk) * plane + own] : 0.0f;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (s[j].role != AA_RECIPIENT) continue;
#pragma unroll
            for (int kk = 0; kk < VA_CHUNK; kk++)
                if (k0 + kk < C) acc[kk] += s[j].weight * (img[(size_t)(k0 + kk) * plane + s[j].other] - cr[kk]);
        }
#pragma unroll
        for (int kk = 0; kk < VA_CHUNK; kk++)
            if (k0 + kk < C) dst[(size_t)(k0 + kk) * plane] = acc[kk];
    }
}

// ---- backward to the image, and dL/dt per near pixel and slot -----------------------------------------------------------------
// grad_images and pair_grads may each be NULL (not both): that result is then not formed
__global__ void __launch_bounds__(256) k_antialias_images_backward(AttrMaps m, AaScene sc, const float* __restrict__ images,
                                                                   int C, const float* __restrict__ grad_out,
                                                                   float* __restrict__ grad_images,
                                                                   float* __restrict__ pair_grads) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    int b, x, y, fn;
    if (!fr_pixel(m, p, b, x, y, fn)) return;
    const int S = m.S;
    const size_t plane = (size_t)S * S, own = (size_t)(S - 1 - y) * S + x;
    AaSlot s[4];
#pragma unroll
    for (int j = 0; j < 4; j++) aa_slot(m, sc, b, x, y, j, s[j]);
    const float* img = images + (size_t)b * C * plane;
    const float* go = grad_out + (size_t)b * C * plane;
    float pg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = 0; k0 < C; k0 += VA_CHUNK) {
        float gr[VA_CHUNK], acc[VA_CHUNK];
#pragma unroll
        for (int kk = 0; kk < VA_CHUNK; kk++) acc[kk] = gr[kk] = k0 + kk < C ? go[(size_t)(k0 + kk) * plane + own] : 0.0f;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (s[j].role == AA_IDLE) continue;
#pragma unroll
            for (int kk = 0; kk < VA_CHUNK; kk++) {
                if (k0 + kk >= C) continue;
                const size_t at = (size_t)(k0 + kk) * plane;
                const float gm = s[j].role == AA_RECIPIENT ? gr[kk] : go[at + s[j].other];        // g_out of the recipient
                acc[kk] += s[j].role == AA_RECIPIENT ? -(s[j].weight * gm) : s[j].weight * gm;
                if (pair_grads && s[j].near) pg[j] += gm * (img[at + own] - img[at + s[j].other]);
            }
        }
        if (grad_images) {
#pragma unroll
            for (int kk = 0; kk < VA_CHUNK; kk++)
                if (k0 + kk < C) grad_images[(size_t)b * C * plane + (size_t)(k0 + kk) * plane + own] = acc[kk];
        }
    }
    if (pair_grads) {
#pragma unroll
        for (int j = 0; j < 4; j++) pair_grads[4 * (size_t)p + j] = pg[j];
    }
}

// ---- backward to the vertices, stage 1: fr_face_sums / fr_large_face_sums (d3m_fragments.h) with nine accumulators -------------
struct AaFaceSums {
    const AttrMaps& m;
    const float* pair_grads;
    float* Gv;
    float face[9];
    float w;
    __device__ __forceinline__ void setup(const float* f, int) {
#pragma unroll
        for (int k = 0; k < 9; k++) face[k] = f[k];
        w = aa_face_sign(f);
    }
    __device__ __forceinline__ void add(int x, int y, size_t q, float* acc) const {
        const int S = m.S;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const float g = pair_grads[4 * q + j];
            if (g == 0.0f) continue;                                      // (not the near pixel, or a pair that does nothing)
            const int axis = j >> 1, up = j & 1;
            const int xo = x + (axis ? 0 : (up ? 1 : -1)), yo = y + (axis ? (up ? 1 : -1) : 0);
            if (xo < 0 || xo >= S || yo < 0 || yo >= S) continue;
            const AaEdge e = aa_exit_edge(face, w, x, y, xo, yo, S);
            if (e.k < 0) continue;
            const float inv = 1.0f / (e.D * e.D);
            const float gN = -g * e.Eo * inv, gE = g * e.N * inv;
            const float pnx = pixel_center(x, S), pny = pixel_center(y, S), pox = pixel_center(xo, S), poy = pixel_center(yo, S);
            const float xa = e.ax, ya = e.ay, xc = e.cx, yc = e.cy;
            const float ta_x = gN * (yc - pny) + gE * (yc - poy), ta_y = gN * (pnx - xc) + gE * (pox - xc);
            const float tc_x = gN * (pny - ya) + gE * (poy - ya), tc_y = gN * (xa - pnx) + gE * (xa - pox);
            const int kc = e.k == 2 ? 0 : e.k + 1;
#pragma unroll
            for (int k = 0; k < 3; k++) {                                 // (selects, not a runtime index: acc stays in registers)
                acc[3 * k + 0] += k == e.k ? ta_x : (k == kc ? tc_x : 0.0f);
                acc[3 * k + 1] += k == e.k ? ta_y : (k == kc ? tc_y : 0.0f);
            }
        }
    }
    __device__ __forceinline__ void store(size_t gi, const float* acc) const {
#pragma unroll
        for (int k = 0; k < 9; k++) Gv[gi * 9 + k] = acc[k];
    }
};

__global__ void __launch_bounds__(256) k_antialias_face_sums(AttrMaps m, const float* __restrict__ pair_grads,
                                                             const int* __restrict__ list, const int* __restrict__ n_list,
                                                             float* __restrict__ Gv) {
    AaFaceSums policy{m, pair_grads, Gv};
    fr_face_sums<9>(m, list, n_list, policy);
}

__global__ void __launch_bounds__(RG_BLOCK) k_antialias_large_face_sums(AttrMaps m, const float* __restrict__ pair_grads,
                                                                       const int* __restrict__ list,
                                                                       const int* __restrict__ n_list, float* __restrict__ Gv) {
    AaFaceSums policy{m, pair_grads, Gv};
    fr_large_face_sums<9>(m, list, n_list, policy);
}

}  // namespace d3m
