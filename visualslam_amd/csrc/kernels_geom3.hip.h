// The 3 x 3 f64 arithmetic, the inlier test and the record walk that the two-view stages share (kernels_epipolar.hip.h,
// kernels_refit.hip.h, kernels_pose.hip.h), each stated once.  Of include/vslam.h this states "two-view geometry" steps 4 (the Jacobi sweeps on F^T F), 5 (the
// normalisation undone: a product L^T F R) and 6 (Frobenius norm, finite and non-zero), and "relative pose and triangulation"
// steps 1 (E = K^T F K: the same product and norm) and 2 (the same sweeps on E^T E).  Every + - * / sqrt is an IEEE operation
// of its own and sums run left to right: the order written here is the ABI's.  Plain C++ - G3 is __host__ __device__ under
// hipcc and nothing elsewhere - so a host compiler runs the same text (tests/geom3_driver.cpp, against tests/epiref.py).
// Device only, further down: what the two least-squares refits share (the block of the ordered sum, the 9 x 9 Jacobi) and what
// the homography stages share (the transfer test, steps 4 - 7 of the homography model).
// The callers differ in one thing, on purpose: k_pose_candidates unrolls the six sweeps fully (UNROLL = 6), k_epi_models
// does not (UNROLL = 1) - it stands at 257 VGPRs, 80 bytes of scratch and 55296 bytes of LDS, and that budget must not grow.
#pragma once
#include <cmath>
#include <cstddef>

#include "vslam_epipolar_plan.h"
#include "vslam_refit_plan.h"  // the block of the ordered sum: REFIT_WG, REFIT_PER_LANE, REFIT_BLOCK
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

// The rotation nearest to M from its two leading eigen-directions (step 5 of the resection section up to and including
// R[i][j]; step 3 of the loop alignment section): the sweeps on M^T M, v1 and v2 the columns of V beside the smallest
// diagonal entry (lowest index on ties), v3 = v1 x v2; u1 = M v1 normalised, u2 = M v2 made orthogonal to u1 and normalised,
// u3 = u1 x u2; R = u1 v1^T + u2 v2^T + u3 v3^T - a proper rotation whatever the sign of det(M), and the rank-2 M of a 3-point
// sample is its normal case.  n = (n1, n2, n3), the norms of M v1, of the orthogonalised M v2 and of M v3; false: n1 or n2 is
// zero or not finite (R is not written; n3 is set only on success).  k_sim3_models calls this; k_res_models keeps the same
// lines in its own body (routed through this function its device code changes: profiles/sim3_isa_identity.txt).
G3 inline void g3_cross(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
G3 inline void g3_mul(const double (&M)[9], const double (&v)[3], double (&w)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = (M[3 * i] * v[0] + M[3 * i + 1] * v[1]) + M[3 * i + 2] * v[2];
}
G3 inline double g3_norm(const double (&w)[3]) { return sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]); }
G3 inline bool g3_nearest_rotation(const double (&M)[9], double (&R)[9], double (&n)[3]) {
    double S[3], V[3][3];
    g3_gram_jacobi<1>(M, S, V);
    int k = 0;
    double smin = S[0];
    if (S[1] < smin) k = 1, smin = S[1];
    if (S[2] < smin) k = 2, smin = S[2];
    double v1[3], v2[3], v3[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        v1[i] = k == 0 ? V[i][1] : V[i][0];
        v2[i] = k == 2 ? V[i][1] : V[i][2];
    }
    g3_cross(v1, v2, v3);
    double w1[3], w2[3], w3[3], u1[3], u2[3], u3[3];
    g3_mul(M, v1, w1);
    n[0] = g3_norm(w1);
    if (!g3_finite_nonzero(n[0])) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) u1[i] = w1[i] / n[0];
    g3_mul(M, v2, w2);
    const double g = (u1[0] * w2[0] + u1[1] * w2[1]) + u1[2] * w2[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) w2[i] = w2[i] - g * u1[i];
    n[1] = g3_norm(w2);
    if (!g3_finite_nonzero(n[1])) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) u2[i] = w2[i] / n[1];
    g3_cross(u1, u2, u3);
    g3_mul(M, v3, w3);
    n[2] = g3_norm(w3);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[3 * i + c] = (u1[i] * v1[c] + u2[i] * v2[c]) + u3[i] * v3[c];
    return true;
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

// What the two least-squares refits share (kernels_refit.hip.h under F, kernels_hrefit.hip.h under (H, G)): one block of the
// ordered sum, the pair's sum of its blocks, and the cyclic Jacobi on the symmetric 9 x 9 moment matrix.
// One block of the ordered sum: member(p) is the stage's membership predicate, add(s, p) adds a member's N terms to the slot's
// sums, in the header's order of records.  STRIDE: the f64 per block of the stage's scratch (its widest pass).
template <int N, int STRIDE, class Member, class Add>
__device__ __forceinline__ void refit_block_sums(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                 double* __restrict__ partial, unsigned int sum_blocks, double* lds, Member member, Add add) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(counts, j, mcap);
    const size_t first = (size_t)blockIdx.x * REFIT_BLOCK;
    const EpiXY* src = xy + (size_t)j * mcap;
    double s[N];
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = 0.0;
#pragma unroll 4
    for (unsigned int k = 0; k < REFIT_PER_LANE; ++k) {
        const size_t i = first + (size_t)k * REFIT_WG + threadIdx.x;
        if (i < m) {
            const EpiXY p = src[i];
            if (member(p)) add(s, p);  // (a record that is not a member adds +0.0: nothing)
        }
    }
    refit_tree<N>(s, lds);
    if (threadIdx.x == 0) {
        double* out = partial + ((size_t)j * sum_blocks + blockIdx.x) * STRIDE;
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = s[k];
    }
}

// The pair's sum of N block sums, ((B_0 + B_1) + B_2) + ...; +0.0 without a block.
template <int N, int STRIDE>
__device__ __forceinline__ void refit_pair_sums(const double* __restrict__ partial, int j, unsigned int sum_blocks, unsigned int m, double (&s)[N]) {
    const unsigned int nb = (unsigned int)(((size_t)m + REFIT_BLOCK - 1) / REFIT_BLOCK);
    const double* src = partial + (size_t)j * sum_blocks * STRIDE;
#pragma unroll
    for (int k = 0; k < N; ++k) s[k] = nb ? src[k] : 0.0;
    for (unsigned int b = 1; b < nb; ++b) {
#pragma unroll
        for (int k = 0; k < N; ++k) s[k] = s[k] + src[(size_t)b * STRIDE + k];
    }
}

// The rest of step 2 of either refit from the pair's two distance sums: false = the normalisation is degenerate (stop 2).
__device__ __forceinline__ bool refit_scales(const double (&s)[2], unsigned int n_cur, double& sq, double& st) {
    const double nd = (double)n_cur;
    const double dq = s[0] / nd, dt = s[1] / nd;
    if (!g3_finite_nonzero(dq) || !g3_finite_nonzero(dt)) return false;
    sq = 1.4142135623730951 / dq;
    st = 1.4142135623730951 / dt;
    return true;
}

// One Jacobi rotation of the pair (P, Q) of the symmetric 9 x 9 S (the upper triangle is kept: S[min][max]).  P and Q are
// compile-time and every loop is unrolled, so S and V never leave the registers.
template <int P, int Q>
__device__ __forceinline__ void refit_rotate(double (&S)[9][9], double (&V)[9][9]) {
    const double apq = S[P][Q];
    if (apq == 0.0) return;
    const double theta = (S[Q][Q] - S[P][P]) / (2.0 * apq);
    const double den = fabs(theta) + sqrt(theta * theta + 1.0);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / den;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    S[P][P] = S[P][P] - t * apq;
    S[Q][Q] = S[Q][Q] + t * apq;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        if (r == P || r == Q) continue;
        double& rp = r < P ? S[r][P] : S[P][r];
        double& rq = r < Q ? S[r][Q] : S[Q][r];
        const double nrp = c * rp - s * rq, nrq = s * rp + c * rq;
        rp = nrp, rq = nrq;
    }
    S[P][Q] = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const double vp = c * V[i][P] - s * V[i][Q], vq = s * V[i][P] + c * V[i][Q];
        V[i][P] = vp, V[i][Q] = vq;
    }
}
template <int P, int Q>
__device__ __forceinline__ void refit_sweep_from(double (&S)[9][9], double (&V)[9][9]) {
    refit_rotate<P, Q>(S, V);
    if constexpr (Q < 8)
        refit_sweep_from<P, Q + 1>(S, V);
    else if constexpr (P < 7)
        refit_sweep_from<P + 1, P + 2>(S, V);
}
// Step 4 of either refit: `sweeps` cyclic sweeps on the upper triangle of S (V comes in as the identity), then f = the column
// of V at the smallest diagonal entry left, the lowest index on ties (a NaN is never smaller).
__device__ __forceinline__ void refit_smallest_eigenvector(double (&S)[9][9], double (&V)[9][9], int sweeps, double (&f)[9]) {
#pragma unroll 1
    for (int sweep = 0; sweep < sweeps; ++sweep) refit_sweep_from<0, 1>(S, V);
    double smin = S[0][0];
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = V[i][0];
#pragma unroll
    for (int k = 1; k < 9; ++k)
        if (S[k][k] < smin) {
            smin = S[k][k];
#pragma unroll
            for (int i = 0; i < 9; ++i) f[i] = V[i][k];
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

// Steps 4 and 5 of the homography model (k_hom_models from its 4 records, k_hrefit_solve from the members): H = Tt^-1 Hn Tq
// with Frobenius norm 1, before the sign; false: the norm is zero or not finite.
__device__ __forceinline__ bool hom_denormalise(const double (&hn)[9], double cqx, double cqy, double sq, double ctx, double cty, double st,
                                                double (&Hc)[9]) {
    const double aq = -(sq * cqx), bq = -(sq * cqy), r = 1.0 / st;
    double G1[9], M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        G1[3 * i] = hn[3 * i] * sq, G1[3 * i + 1] = hn[3 * i + 1] * sq;
        G1[3 * i + 2] = (hn[3 * i] * aq + hn[3 * i + 1] * bq) + hn[3 * i + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        M[c] = r * G1[c] + ctx * G1[6 + c];
        M[3 + c] = r * G1[3 + c] + cty * G1[6 + c];
        M[6 + c] = G1[6 + c];
    }
    const double nrm = g3_frobenius(M);
    if (!g3_finite_nonzero(nrm)) return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) Hc[i] = M[i] / nrm;
    return true;
}
// Step 6: H's sign from the query point (x0, y0) that must map to the front; false: neither w > 0 nor w < 0.
__device__ __forceinline__ bool hom_sign(double (&Hc)[9], double x0, double y0) {
    const double w = (Hc[6] * x0 + Hc[7] * y0) + Hc[8];
    if (!(w > 0.0) && !(w < 0.0)) return false;
    if (w < 0.0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) Hc[i] = -Hc[i];
    }
    return true;
}
// Step 7: G = adj(H) with its sign from the train point (u0, v0); false: wg is zero or not finite.
__device__ __forceinline__ bool hom_adjugate(const double (&Hc)[9], double u0, double v0, double (&Gc)[9]) {
    Gc[0] = Hc[4] * Hc[8] - Hc[5] * Hc[7], Gc[1] = Hc[2] * Hc[7] - Hc[1] * Hc[8], Gc[2] = Hc[1] * Hc[5] - Hc[2] * Hc[4];
    Gc[3] = Hc[5] * Hc[6] - Hc[3] * Hc[8], Gc[4] = Hc[0] * Hc[8] - Hc[2] * Hc[6], Gc[5] = Hc[2] * Hc[3] - Hc[0] * Hc[5];
    Gc[6] = Hc[3] * Hc[7] - Hc[4] * Hc[6], Gc[7] = Hc[1] * Hc[6] - Hc[0] * Hc[7], Gc[8] = Hc[0] * Hc[4] - Hc[1] * Hc[3];
    const double wg = (Gc[6] * u0 + Gc[7] * v0) + Gc[8];
    if (!g3_finite_nonzero(fabs(wg))) return false;
    if (wg < 0.0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) Gc[i] = -Gc[i];
    }
    return true;
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
