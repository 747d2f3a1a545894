// The kernel bodies of csrc/d3m_pose.h on the host, under the address and undefined-behaviour sanitizers.  Integer inputs
// with all angles 0 (the generators of tests/test_gpu_pose.py): every output and gradient must equal the integer answer
// exactly at every shape, with every array a heap block of its exact size, so an access outside it is reported.  One float
// case: the gradient of the pose against central differences of a double restatement.  See run.sh.
#include "d3m_pose.h"
#include <cstdio>
#include <cstdlib>
#include <vector>
using namespace d3m;

static long hash(long r, long k, long salt) { return (r * 1315423911L + k * 2654435761L + salt * 97531L) % 65521L; }
static long hashed_int(long r, long k, long salt, long lo, long hi) { return hash(r, k, salt) * (hi - lo + 1) / 65521 + lo; }
static float hashed_float(long r, long k, long salt, double lo, double hi) { return (float)(lo + (hi - lo) * (hash(r, k, salt) / 65520.0)); }

template <class T>
struct Block {          // a heap block of exactly n elements (none: NULL)
    T* p;
    explicit Block(size_t n) : p(n ? (T*)malloc(n * sizeof(T)) : nullptr) {}
    ~Block() { free(p); }
    Block(const Block&) = delete;
};

struct Case {
    int V, B, L, shared, use_posed, use_uv, use_lm;
};

// d3m_pose_forward / d3m_pose_backward of csrc/d3m_raster.hip, launch for launch
static void forward(const float* x, int vb, const float* pose, int stride, float tau, float limit, float uv_size, const int32_t* lmk,
                    int L, float* posed, float* uv, float* lm, int B, int V) {
    const long items = ((posed || uv) ? V : 0) + (lm ? L : 0);
    launch(dim3(pose_parts(items), B), dim3(PS_BLOCK),
           [=] { k_pose_forward(x, vb, pose, stride, tau, limit, uv_size, lmk, L, posed, uv, lm, V); });
}
static void backward(const float* x, int vb, const float* pose, int stride, float tau, float limit, float uv_size,
                     const int32_t* lmk, int L, const float* g_posed, const float* g_uv, const float* g_lm, float* scratch,
                     float* g_x, float* g_pose, int B, int V) {
    const bool dense = g_posed || g_uv, chunks = g_x || dense;
    const int parts = dense && g_pose ? pose_parts(V) : 0;
    if (chunks)
        launch(dim3(pose_parts(V), vb > 1 ? B : 1), dim3(PS_BLOCK), [=] {
            k_pose_backward_chunks(x, vb, pose, stride, limit, uv_size, g_posed, g_uv, g_x, parts > 0 ? scratch : nullptr, B, V);
        });
    const int pose_blocks = g_pose ? (B + PS_FINISH_SETS - 1) / PS_FINISH_SETS : 0;
    const int lm_blocks = !(g_lm && g_x) ? 0 : (vb > 1 ? (3 * B + PS_FINISH_SETS - 1) / PS_FINISH_SETS : 1);
    if (pose_blocks + lm_blocks > 0)
        launch(dim3(pose_blocks + lm_blocks), dim3(PS_FINISH_SETS), [=] {
            k_pose_backward_finish(x, vb, pose, stride, tau, limit, lmk, L, g_lm, scratch, parts, g_x, g_pose, B, V, pose_blocks);
        });
}

static int run_integers(const Case& c, int pose_stride) {
    const int V = c.V, B = c.B, L = c.use_lm ? c.L : 0, vb = c.shared ? 1 : B;
    const float tau = 4.f, uv_size = 1.f;
    Block<float> x((size_t)vb * V * 3), pose((size_t)(B - 1) * pose_stride + 7), posed(c.use_posed ? (size_t)B * V * 3 : 0),
        uv(c.use_uv ? (size_t)B * V * 2 : 0), lm((size_t)B * L * 3), g_posed(c.use_posed ? (size_t)B * V * 3 : 0),
        g_uv(c.use_uv ? (size_t)B * V * 2 : 0), g_lm((size_t)B * L * 3), g_x((size_t)vb * V * 3), g_pose((size_t)B * 7),
        scratch((size_t)B * pose_parts(V) * PS_SUMS);
    Block<int32_t> lmk(L);
    for (long i = 0; i < (long)vb * V; i++)
        for (int k = 0; k < 3; k++) x.p[i * 3 + k] = (float)hashed_int(i, k, 101, -3, 3);
    for (size_t i = 0; i < (size_t)(B - 1) * pose_stride + 7; i++) pose.p[i] = NAN;      // (the gaps of a strided pose are never read)
    for (int b = 0; b < B; b++) {
        float* p = pose.p + (size_t)b * pose_stride;
        p[0] = (float)hashed_int(b, 0, 102, -2, 2);
        p[1] = p[2] = p[3] = 0.f;
        for (int k = 0; k < 3; k++) p[4 + k] = (float)hashed_int(b, k, 103, -5, 5);
    }
    for (long i = 0; i < (long)B * V; i++) {
        for (int k = 0; k < 3; k++) if (g_posed.p) g_posed.p[i * 3 + k] = (float)hashed_int(i, k, 104, -2, 2);
        for (int k = 0; k < 2; k++) if (g_uv.p) g_uv.p[i * 2 + k] = (float)hashed_int(i, k, 105, -2, 2);
    }
    for (int l = 0; l < L; l++) lmk.p[l] = (int32_t)((hash(l, 0, 300) * 31 + (long)l * 7919) % V);
    if (L == 300)
        for (int l = L - 1; l >= 3; l--) if (l % 3 == 0) lmk.p[l] = lmk.p[l - 3];     // repeats
    for (long i = 0; i < (long)B * L; i++)
        for (int k = 0; k < 3; k++) g_lm.p[i * 3 + k] = (float)hashed_int(i, k, 106, -2, 2);
    for (size_t i = 0; i < (size_t)vb * V * 3; i++) g_x.p[i] = NAN;
    for (int i = 0; i < B * 7; i++) g_pose.p[i] = NAN;
    for (size_t i = 0; i < (size_t)B * pose_parts(V) * PS_SUMS; i++) scratch.p[i] = NAN;

    forward(x.p, vb, pose.p, pose_stride, tau, 0.f, uv_size, lmk.p, L, posed.p, uv.p, lm.p, B, V);
    backward(x.p, vb, pose.p, pose_stride, tau, 0.f, uv_size, lmk.p, L, g_posed.p, g_uv.p, g_lm.p, scratch.p, g_x.p, g_pose.p, B, V);

    long bad = 0;
    std::vector<long> G((size_t)B * V * 3, 0), gx((size_t)vb * V * 3, 0);
    for (int b = 0; b < B; b++) {
        const float* p = pose.p + (size_t)b * pose_stride;
        const long s = (long)p[0];
        auto want = [&](int v, int k) { return s * (long)x.p[((size_t)(c.shared ? 0 : b) * V + v) * 3 + k] + 4 * (long)p[4 + k]; };
        for (int v = 0; v < V; v++) {
            const size_t at = (size_t)b * V + v;
            for (int k = 0; k < 3; k++) {
                if (posed.p) bad += posed.p[at * 3 + k] != (float)want(v, k);
                if (g_posed.p) G[at * 3 + k] += (long)g_posed.p[at * 3 + k];
            }
            if (uv.p) {
                bad += uv.p[at * 2] != (float)want(v, 0);
                bad += uv.p[at * 2 + 1] != (float)(1 - want(v, 1));
                G[at * 3] += (long)g_uv.p[at * 2];
                G[at * 3 + 1] -= (long)g_uv.p[at * 2 + 1];
            }
        }
        for (int l = 0; l < L; l++)
            for (int k = 0; k < 3; k++) {
                bad += lm.p[((size_t)b * L + l) * 3 + k] != (float)want(lmk.p[l], k);
                G[((size_t)b * V + lmk.p[l]) * 3 + k] += (long)g_lm.p[((size_t)b * L + l) * 3 + k];
            }
        long M[9] = {0}, n[3] = {0};
        for (int v = 0; v < V; v++)
            for (int j = 0; j < 3; j++) {
                const long g = G[((size_t)b * V + v) * 3 + j];
                n[j] += g;
                gx[((size_t)(c.shared ? 0 : b) * V + v) * 3 + j] += s * g;
                for (int k = 0; k < 3; k++) M[3 * j + k] += g * (long)x.p[((size_t)(c.shared ? 0 : b) * V + v) * 3 + k];
            }
        const long wp[7] = {M[0] + M[4] + M[8], s * (M[7] - M[5]), s * (M[2] - M[6]), s * (M[3] - M[1]), 4 * n[0], 4 * n[1], 4 * n[2]};
        for (int k = 0; k < 7; k++) bad += g_pose.p[b * 7 + k] != (float)wp[k];
    }
    for (size_t i = 0; i < (size_t)vb * V * 3; i++) bad += g_x.p[i] != (float)gx[i];
    printf("V=%d B=%d L=%d shared=%d outputs=%d%d%d stride=%d: %s\n", V, B, L, c.shared, c.use_posed, c.use_uv, c.use_lm, pose_stride,
           bad ? "MISMATCH" : "exact");
    return bad != 0;
}

// One float case: grad_pose and grad_vertices against central differences of the double restatement.
static double loss(int B, int V, int L, int shared, const double* x, const double* pose, double tau, double limit, double uv_size,
                   const int32_t* lmk, const float* g_posed, const float* g_uv, const float* g_lm) {
    double total = 0;
    for (int b = 0; b < B; b++) {
        const double* p = pose + b * 7;
        double a[3], c[3], s[3];
        for (int k = 0; k < 3; k++) { a[k] = std::min(std::max(p[1 + k], -limit), limit); c[k] = cos(a[k]); s[k] = sin(a[k]); }
        const double rx[9] = {1, 0, 0, 0, c[0], -s[0], 0, s[0], c[0]}, ry[9] = {c[1], 0, s[1], 0, 1, 0, -s[1], 0, c[1]},
                     rz[9] = {c[2], -s[2], 0, s[2], c[2], 0, 0, 0, 1};
        double xy[9], r[9];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { xy[3 * i + j] = 0; for (int k = 0; k < 3; k++) xy[3 * i + j] += rx[3 * i + k] * ry[3 * k + j]; }
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { r[3 * i + j] = 0; for (int k = 0; k < 3; k++) r[3 * i + j] += xy[3 * i + k] * rz[3 * k + j]; }
        auto point = [&](int v, double* out) {
            const double* q = x + ((size_t)(shared ? 0 : b) * V + v) * 3;
            for (int j = 0; j < 3; j++) out[j] = p[0] * (r[3 * j] * q[0] + r[3 * j + 1] * q[1] + r[3 * j + 2] * q[2]) + tau * p[4 + j];
        };
        double q[3];
        for (int v = 0; v < V; v++) {
            point(v, q);
            const size_t at = (size_t)b * V + v;
            for (int j = 0; j < 3; j++) total += g_posed[at * 3 + j] * q[j];
            total += g_uv[at * 2] * (q[0] / uv_size) + g_uv[at * 2 + 1] * (1 - q[1] / uv_size);
        }
        for (int l = 0; l < L; l++) {
            point(lmk[l], q);
            for (int j = 0; j < 3; j++) total += g_lm[((size_t)b * L + l) * 3 + j] * q[j];
        }
    }
    return total;
}

static int run_floats(int shared) {
    const int V = 2 * PS_BLOCK + 3, B = 3, L = 7, vb = shared ? 1 : B;
    const float tau = 5.f, limit = 3.1415f, uv_size = 7.f;
    Block<float> x((size_t)vb * V * 3), pose(B * 7), g_posed((size_t)B * V * 3), g_uv((size_t)B * V * 2), g_lm(B * L * 3),
        g_x((size_t)vb * V * 3), g_pose(B * 7), scratch((size_t)B * pose_parts(V) * PS_SUMS);
    Block<int32_t> lmk(L);
    for (size_t i = 0; i < (size_t)vb * V * 3; i++) x.p[i] = hashed_float(i, 0, 1, -2, 2);
    for (int i = 0; i < B * 7; i++) pose.p[i] = hashed_float(i, 0, 2, -1.5, 1.5);
    pose.p[1] = 3.3f;                                       // beyond the limit: clamped, no gradient
    for (size_t i = 0; i < (size_t)B * V * 3; i++) g_posed.p[i] = hashed_float(i, 0, 3, -1, 1);
    for (size_t i = 0; i < (size_t)B * V * 2; i++) g_uv.p[i] = hashed_float(i, 0, 4, -1, 1);
    for (int i = 0; i < B * L * 3; i++) g_lm.p[i] = hashed_float(i, 0, 5, -1, 1);
    for (int l = 0; l < L; l++) lmk.p[l] = (int32_t)((hash(l, 0, 6) * 31) % V);
    lmk.p[L - 1] = lmk.p[0];
    backward(x.p, vb, pose.p, 7, tau, limit, uv_size, lmk.p, L, g_posed.p, g_uv.p, g_lm.p, scratch.p, g_x.p, g_pose.p, B, V);
    std::vector<double> xd(x.p, x.p + (size_t)vb * V * 3), pd(pose.p, pose.p + B * 7);
    auto f = [&] { return loss(B, V, L, shared, xd.data(), pd.data(), tau, limit, uv_size, lmk.p, g_posed.p, g_uv.p, g_lm.p); };
    int bad = 0;
    const double h = 1e-6;
    double scale = 0;
    for (int i = 0; i < B * 7; i++) scale = std::max(scale, (double)fabsf(g_pose.p[i]));
    for (int i = 0; i < B * 7; i++) {
        const double keep = pd[i];
        pd[i] = keep + h; const double up = f();
        pd[i] = keep - h; const double down = f();
        pd[i] = keep;
        const double fd = (up - down) / (2 * h);
        if (fabs(fd - g_pose.p[i]) > 1e-4 * scale) { printf("  grad_pose[%d] = %g, central difference %g\n", i, g_pose.p[i], fd); bad++; }
    }
    bad += g_pose.p[1] != 0.f;
    for (size_t i = 0; i < (size_t)vb * V * 3; i += 97) {
        const double keep = xd[i];
        xd[i] = keep + h; const double up = f();
        xd[i] = keep - h; const double down = f();
        xd[i] = keep;
        const double fd = (up - down) / (2 * h);
        if (fabs(fd - g_x.p[i]) > 1e-4 * std::max(1.0, fabs(fd))) { printf("  grad_vertices[%zu] = %g, central difference %g\n", i, g_x.p[i], fd); bad++; }
    }
    printf("float case, shared=%d: %s\n", shared, bad ? "MISMATCH" : "gradients agree with central differences");
    return bad != 0;
}

int main() {
    int bad = 0, cases = 0;
    const int Vs[] = {1, 63, 64, 65, PS_BLOCK - 1, PS_BLOCK, 2 * PS_BLOCK + 3, PS_BLOCK * PS_MAX_PARTS + 5};
    const int modes[][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {1, 1, 1}};
    for (int V : Vs)
        for (int B : {1, 3, PS_FINISH_SETS + 1}) {
            if (B > 3 && V > 2 * PS_BLOCK + 3) continue;    // (minutes on the host's threads, and no other path)
            for (int shared = 0; shared < 2; shared++)
                for (int L : {0, 1, 68, 300})
                    for (auto& m : modes) {
                        if ((m[2] && !m[0] && L == 0) || (!m[2] && L > 0)) continue;
                        bad += run_integers(Case{V, B, L, shared, m[0], m[1], m[2] && L > 0}, 7);
                        cases++;
                    }
        }
    bad += run_integers(Case{2 * PS_BLOCK + 3, 3, 68, 0, 1, 1, 1}, 235); cases++;
    bad += run_floats(0) + run_floats(1); cases += 2;
    printf("%d cases, %d failing\n", cases, bad);
    return bad != 0;
}
