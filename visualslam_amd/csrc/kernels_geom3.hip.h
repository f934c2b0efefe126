// The 3 x 3 f64 arithmetic, the inlier test and the record walk that the two-view stages share (kernels_epipolar.hip.h,
// kernels_refit.hip.h, kernels_pose.hip.h), each stated once.  Of include/vslam.h this states "two-view geometry" steps 4 (the Jacobi sweeps on F^T F), 5 (the
// normalisation undone: a product L^T F R) and 6 (Frobenius norm, finite and non-zero), and "relative pose and triangulation"
// steps 1 (E = K^T F K: the same product and norm) and 2 (the same sweeps on E^T E).  Every + - * / sqrt is an IEEE operation
// of its own and sums run left to right: the order written here is the ABI's.  Plain C++ - G3 is __host__ __device__ under
// hipcc and nothing elsewhere - so a host compiler runs the same text (tests/geom3_driver.cpp, against tests/epiref.py).
// The callers differ in one thing, on purpose: k_pose_candidates unrolls the six sweeps fully (UNROLL = 6), k_epi_models
// does not (UNROLL = 1) - it stands at 257 VGPRs, 80 bytes of scratch and 55296 bytes of LDS, and that budget must not grow.
#pragma once
#include <cmath>
#include <cstddef>

#include "vslam_epipolar_plan.h"
#ifdef __HIPCC__
#define G3 __host__ __device__
#else
#define G3
#endif

namespace vslam {

G3 inline bool g3_finite_nonzero(double n) { return n != 0.0 && n < __builtin_huge_val(); }

// One Jacobi rotation of the pair (P, Q) of a symmetric 3 x 3 S: app, aqq, apq its block, arp, arq the third index's two
// entries.  P and Q are compile-time, so V never leaves the registers.
template <int P, int Q>
G3 inline void g3_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double (&V)[3][3]) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double den = fabs(theta) + sqrt(theta * theta + 1.0);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / den;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double napp = app - t * apq, naqq = aqq + t * apq;
    const double narp = c * arp - s * arq, narq = s * arp + c * arq;
    app = napp, aqq = naqq, apq = 0.0, arp = narp, arq = narq;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double vp = c * V[i][P] - s * V[i][Q], vq = s * V[i][P] + c * V[i][Q];
        V[i][P] = vp, V[i][Q] = vq;
    }
}

// S = M^T M of the row-major M, six cyclic sweeps (0, 1), (0, 2), (1, 2): d = the diagonal left, V = the rotations accumulated.
template <int UNROLL>
G3 inline void g3_gram_jacobi(const double (&M)[9], double (&d)[3], double (&V)[3][3]) {
    double S00 = (M[0] * M[0] + M[3] * M[3]) + M[6] * M[6], S01 = (M[0] * M[1] + M[3] * M[4]) + M[6] * M[7],
           S02 = (M[0] * M[2] + M[3] * M[5]) + M[6] * M[8], S11 = (M[1] * M[1] + M[4] * M[4]) + M[7] * M[7],
           S12 = (M[1] * M[2] + M[4] * M[5]) + M[7] * M[8], S22 = (M[2] * M[2] + M[5] * M[5]) + M[8] * M[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i / 3][i % 3] = i / 3 == i % 3 ? 1.0 : 0.0;
#pragma unroll UNROLL
    for (int sweep = 0; sweep < 6; ++sweep) {
        g3_rotate<0, 1>(S00, S11, S01, S02, S12, V);
        g3_rotate<0, 2>(S00, S22, S02, S01, S12, V);
        g3_rotate<1, 2>(S11, S22, S12, S01, S02, V);
    }
    d[0] = S00, d[1] = S11, d[2] = S22;
}

// Rank 2 (step 4 of the two-view model): the right singular vector of f's smallest singular value is projected out of
// every row.  (The refit's k_refit_solve; k_epi_models keeps the same lines in its own body: routed through this function
// its register allocation changes, and its budget - above - must not.)
G3 inline void g3_rank2(double (&f)[9]) {
    double S[3], V[3][3];
    g3_gram_jacobi<1>(f, S, V);
    double v0 = V[0][0], v1 = V[1][0], v2 = V[2][0], smin = S[0];
    if (S[1] < smin) v0 = V[0][1], v1 = V[1][1], v2 = V[2][1], smin = S[1];
    if (S[2] < smin) v0 = V[0][2], v1 = V[1][2], v2 = V[2][2], smin = S[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double g = (f[3 * i] * v0 + f[3 * i + 1] * v1) + f[3 * i + 2] * v2;
        f[3 * i] = f[3 * i] - g * v0;
        f[3 * i + 1] = f[3 * i + 1] - g * v1;
        f[3 * i + 2] = f[3 * i + 2] - g * v2;
    }
}

struct G3Affine {  // the matrix [[sx, 0, ax], [0, sy, ay], [0, 0, 1]]: a normalisation, or the intrinsics
    double sx, sy, ax, ay;
};
// out = L^T F R, the right factor first.
G3 inline void g3_lt_f_r(const G3Affine& L, const double (&F)[9], const G3Affine& R, double (&out)[9]) {
    double G[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        G[3 * i] = F[3 * i] * R.sx, G[3 * i + 1] = F[3 * i + 1] * R.sy;
        G[3 * i + 2] = (F[3 * i] * R.ax + F[3 * i + 1] * R.ay) + F[3 * i + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out[c] = L.sx * G[c], out[3 + c] = L.sy * G[3 + c];
        out[6 + c] = (L.ax * G[c] + L.ay * G[3 + c]) + G[6 + c];
    }
}

// The Frobenius norm, the squares summed left to right.
G3 inline double g3_frobenius(const double (&M)[9]) {
    double n2 = M[0] * M[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) n2 = n2 + M[i] * M[i];
    return sqrt(n2);
}

// The Sampson test of one record under F (the two-view section's inlier test); false for NaN coordinates, for a zero
// denominator and for F = 0.  (k_epi_score, k_epi_flags and the refit's streaming kernels.)
G3 inline bool epi_inlier(const double (&F)[9], const EpiXY& p, double max_dist2) {
    const double a0 = (F[0] * p.x + F[1] * p.y) + F[2], a1 = (F[3] * p.x + F[4] * p.y) + F[5], a2 = (F[6] * p.x + F[7] * p.y) + F[8];
    const double b0 = (F[0] * p.u + F[3] * p.v) + F[6], b1 = (F[1] * p.u + F[4] * p.v) + F[7];
    const double e = (p.u * a0 + p.v * a1) + a2;
    const double den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
    return e * e < max_dist2 * den;
}

// The counter hash of the sampling (the two-view section's mix(); k_epi_models and k_hom_models).
G3 inline unsigned int epi_mix(unsigned int x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// The record walk.  Pair j has min(count, capacity) records; lane `lane` of workgroup `block` has record i, 64 bits (the last
// block of a capacity near 2^32 runs past it); a wave none of whose records lies below m leaves (wave-uniform); lane 0 of a
// wave speaks for it and stores its ballot word, word i / 64 of pair j.
G3 inline unsigned int g3_count(const unsigned int* __restrict__ counts, int j, unsigned int cap) { return counts[j] < cap ? counts[j] : cap; }
G3 inline size_t g3_record(unsigned int block, unsigned int wg, unsigned int lane) { return (size_t)block * wg + lane; }
G3 inline bool g3_wave_has_record(size_t i, unsigned int m) { return (i & ~(size_t)63) < m; }
G3 inline bool g3_first_lane(unsigned int lane) { return (lane & 63) == 0; }
G3 inline void g3_store_word(unsigned long long* words, size_t j, unsigned int fwords, size_t i, bool store, unsigned long long w) {
    if (store) words[j * fwords + (i >> 6)] = w;
}

#ifdef __HIPCC__
// The tree of the ordered sum (the refit section's SUM) over the 256 slots of a workgroup, N sums at once: h = 128 and 64 through LDS (lds [N][128] f64, slot-major:
// the lanes of one access hit consecutive f64), h = 32 .. 1 by __shfl_down inside wave 0.  Lane 0 ends with B_b.
template <int N>
__device__ __forceinline__ void refit_tree(double (&s)[N], double* lds) {
    const unsigned int l = threadIdx.x;
    if (l >= 128) {
#pragma unroll
        for (int k = 0; k < N; ++k) lds[k * 128 + (l - 128)] = s[k];
    }
    __syncthreads();
    if (l < 128) {
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] = s[k] + lds[k * 128 + l];
    }
    __syncthreads();
    if (l >= 64 && l < 128) {
#pragma unroll
        for (int k = 0; k < N; ++k) lds[k * 128 + (l - 64)] = s[k];
    }
    __syncthreads();
    if (l < 64) {
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] = s[k] + lds[k * 128 + l];
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) {
#pragma unroll
            for (int k = 0; k < N; ++k) s[k] = s[k] + __shfl_down(s[k], h);
        }
    }
}

// What the homography, pose and pose-from-homography kernels share per record (kernels_homography.hip.h, kernels_pose.hip.h,
// kernels_hpose.hip.h): the symmetric transfer test and the two-ray solve, each stated once.
// The inlier test of one record under (H, G); false for NaN coordinates (p2 > 0 fails) and for H = G = 0.
__device__ __forceinline__ bool hom_inlier(const double (&H)[9], const double (&G)[9], const EpiXY& p, double max_dist2) {
    const double p0 = (H[0] * p.x + H[1] * p.y) + H[2], p1 = (H[3] * p.x + H[4] * p.y) + H[5], p2 = (H[6] * p.x + H[7] * p.y) + H[8];
    const double q0 = (G[0] * p.u + G[1] * p.v) + G[2], q1 = (G[3] * p.u + G[4] * p.v) + G[5], q2 = (G[6] * p.u + G[7] * p.v) + G[8];
    const double dx = p0 - p.u * p2, dy = p1 - p.v * p2;
    const double ex = q0 - p.x * q2, ey = q1 - p.y * q2;
    const bool fwd = p2 > 0.0 && dx * dx + dy * dy < max_dist2 * (p2 * p2);
    const bool bwd = q2 > 0.0 && ex * ex + ey * ey < max_dist2 * (q2 * q2);
    return fwd && bwd;
}

// The two rays of one record (step 5): q = (q0, q1, 1), b = (b0, b1, 1).
struct PoseRays {
    double q0, q1, b0, b1;
};
__device__ __forceinline__ PoseRays pose_rays(const EpiXY& p, const vslam_pose_params& K) {
    return PoseRays{(p.x - K.cx) / K.fx, (p.y - K.cy) / K.fy, (p.u - K.cx) / K.fx, (p.v - K.cy) / K.fy};
}

// det, n1, n2 of one record under (R, t) (step 5; the third component of q and b is 1, and x * 1 is x).
__device__ __forceinline__ void pose_solve(const double (&R)[9], const double (&t)[3], const PoseRays& r, double& det, double& n1, double& n2) {
    const double a0 = (R[0] * r.q0 + R[1] * r.q1) + R[2], a1 = (R[3] * r.q0 + R[4] * r.q1) + R[5], a2 = (R[6] * r.q0 + R[7] * r.q1) + R[8];
    const double aa = (a0 * a0 + a1 * a1) + a2 * a2;
    const double bb = (r.b0 * r.b0 + r.b1 * r.b1) + 1.0;
    const double ab = (a0 * r.b0 + a1 * r.b1) + a2;
    const double at = (a0 * t[0] + a1 * t[1]) + a2 * t[2];
    const double bt = (r.b0 * t[0] + r.b1 * t[1]) + t[2];
    det = aa * bb - ab * ab;
    n1 = ab * bt - bb * at;
    n2 = aa * bt - ab * at;
}

// A NaN leaves as the quiet NaN 0x7ff8000000000000: IEEE fixes neither the sign nor the payload of a NaN an operation makes.
// (k_pose_points and the trajectory kernels, kernels_chain.hip.h.)
__device__ __forceinline__ double pose_canonical(double x) { return x == x ? x : __longlong_as_double(0x7ff8000000000000ll); }
#endif

}  // namespace vslam
