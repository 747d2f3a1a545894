// The kernel bodies of csrc/d3m_morphable.h on the host, under the address and undefined-behaviour sanitizers, on the integer
// inputs of tests/test_gpu_morphable.py (the same hash): forward and adjoint must equal the integer result exactly at
// every shape, and every array is a heap block of its exact size, so an access outside it is reported.  See run.sh.
#include "d3m_morphable.h"
#include <cstdio>
#include <cstdlib>
using namespace d3m;

static long hash(long r, long k, long salt) { return (r * 1315423911L + k * 2654435761L + salt * 97531L) % 65521L; }
static long hashed_int(long r, long k, long salt, long lo, long hi) { return hash(r, k, salt) * (hi - lo + 1) / 65521 + lo; }

template <int NB>
static void forward(dim3 g, const float* basis, const float* c, const float* mean, float* out, int B, int R, int K, int vec) {
    launch(g, dim3(MB_BLOCK), [=] { k_morphable_forward<NB>(basis, c, mean, nullptr, out, B, R, K, vec); });
}
template <int NB>
static void adjoint(dim3 g, const float* basis, const float* go, float* part, int B, int R, int K) {
    launch(g, dim3(MB_BLOCK), [=] { k_morphable_adjoint_chunks<NB>(basis, go, part, B, R, K); });
}

static int run(int R, int K, int B, int misalign) {
    float* room = (float*)aligned_alloc(16, ((size_t)R * K + 4 + 3) / 4 * 16);
    float* basis = room + (misalign ? 1 : 0);
    float* c = (float*)malloc(sizeof(float) * B * K);
    float* go = (float*)malloc(sizeof(float) * B * R);
    float* mean = (float*)malloc(sizeof(float) * R);
    float* out = (float*)malloc(sizeof(float) * B * R);
    float* gc = (float*)malloc(sizeof(float) * B * K);
    const int n_chunks = (R + MB_ROWS - 1) / MB_ROWS;
    float* part = (float*)aligned_alloc(16, ((size_t)n_chunks * B * K * 4 + 15) / 16 * 16);
    for (int r = 0; r < R; r++) {
        mean[r] = (float)hashed_int(r, 0, 44, -4000, 4000);
        for (int k = 0; k < K; k++) basis[(size_t)r * K + k] = (float)hashed_int(r, k, 41, -3, 3);
    }
    for (int b = 0; b < B; b++) {
        for (int k = 0; k < K; k++) c[b * K + k] = (float)hashed_int(b, k, 42, -2, 2);
        for (int r = 0; r < R; r++) go[(size_t)b * R + r] = (float)hashed_int(r, b, 43, -2, 2);
    }
    for (size_t i = 0; i < (size_t)n_chunks * B * K; i++) part[i] = NAN;
    for (int i = 0; i < B * R; i++) out[i] = NAN;
    for (int i = 0; i < B * K; i++) gc[i] = NAN;
    const int vec = (K % 4 == 0) && (((uintptr_t)basis & 15) == 0);
    const dim3 gf((R + MB_FWD_ROWS - 1) / MB_FWD_ROWS, (B + MB_SETS - 1) / MB_SETS);
    const dim3 ga(n_chunks, (K + MB_KW - 1) / MB_KW, (B + MB_SETS - 1) / MB_SETS);
    if (B == 1) { forward<1>(gf, basis, c, mean, out, B, R, K, vec); adjoint<1>(ga, basis, go, part, B, R, K); }
    else if (B <= 4) { forward<4>(gf, basis, c, mean, out, B, R, K, vec); adjoint<4>(ga, basis, go, part, B, R, K); }
    else { forward<16>(gf, basis, c, mean, out, B, R, K, vec); adjoint<16>(ga, basis, go, part, B, R, K); }
    launch(dim3((K + 63) / 64, B), dim3(MB_FINISH_GROUPS * 64),
           [=] { k_morphable_adjoint_finish(part, n_chunks, nullptr, nullptr, gc, B, K, 0); });
    int bad = 0;
    for (int b = 0; b < B; b++)
        for (int r = 0; r < R; r++) {
            long s = (long)mean[r];
            for (int k = 0; k < K; k++) s += (long)basis[(size_t)r * K + k] * (long)c[b * K + k];
            bad += out[(size_t)b * R + r] != (float)s;
        }
    for (int b = 0; b < B; b++)
        for (int k = 0; k < K; k++) {
            long s = 0;
            for (int r = 0; r < R; r++) s += (long)basis[(size_t)r * K + k] * (long)go[(size_t)b * R + r];
            bad += gc[b * K + k] != (float)s;
        }
    printf("R=%d K=%d B=%d misaligned=%d vec=%d: %s\n", R, K, B, misalign, vec, bad ? "MISMATCH" : "exact");
    free(room); free(c); free(go); free(mean); free(out); free(gc); free(part);
    return bad;
}

int main() {
    int bad = 0, cases = 0;
    const int Rs[] = {1, MB_ROWS - 1, MB_ROWS, 2 * MB_ROWS + 3}, Ks[] = {1, 5, 64, 65, 228, 2 * MB_KW + 1}, Bs[] = {1, 3, MB_SETS, MB_SETS + 1};
    for (int R : Rs) for (int K : Ks) for (int B : Bs) { bad += run(R, K, B, 0); cases++; }
    bad += run(2 * MB_ROWS + 3, 228, 3, 1); bad += run(2 * MB_ROWS + 3, 64, MB_SETS + 1, 1); cases += 2;
    printf("%d cases, %d mismatching elements\n", cases, bad);
    return bad != 0;
}
