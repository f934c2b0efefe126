// Pose from homography (include/vslam.h, "pose from homography"): from the homography of every selected pair and a match list
// to (R, t), the plane's normal and the 3-D point of every record H supports.
//   k_hpose_candidates : one lane per pair: A = K^-1 H K, the eigenvectors of A^T A by the Jacobi sweeps of the two-view model,
//                        the kind, and the four (R, t, n) candidates (steps 1 - 4); everything in registers, statically indexed
//   k_hpose_vote       : the hot path, one lane per match record: H's symmetric transfer test, then the cheirality and the
//                        normal's sign under both rotations - the sign of (t, n) flips n1, n2 and nq exactly, so two evaluations
//                        give all four votes; ballot + popcount per wave, one integer atomicAdd per wave and counter
//   k_hpose_select     : one lane per pair: the winner, the ambiguity rule, the prior (step 6)
//   k_hpose_points     : one lane per record: the midpoint of the two rays under the pose written, and the wave's ballot word
// The {x, y, x', y'} records come from k_epi_coords (vslam::enqueue_epi_coords).  The arithmetic is the header's, operation
// for operation, under the rules of kernels_epipolar.hip.h.  The transfer test (hom_inlier) and the two-ray solve (pose_rays,
// pose_solve) are kernels_geom3.hip.h's, shared with k_hom_score / k_hom_flags and k_pose_vote / k_pose_points.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_geom3.hip.h"
#include "vslam_hpose_plan.h"

namespace vslam {

__device__ __forceinline__ void hp_cross(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double hp_norm(const double (&w)[3]) { return sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]); }
__device__ __forceinline__ void hp_mul(const double (&A)[9], const double (&v)[3], double (&o)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = (A[3 * i] * v[0] + A[3 * i + 1] * v[1]) + A[3 * i + 2] * v[2];
}
// One conditional exchange of step 2: positions A_ < B_ of d, and the same columns of V, change places iff d[B_] > d[A_].
// Two-way selects between registers, as in k_pose_candidates: a column picked by a run-time index would put V in scratch.
template <int A_, int B_>
__device__ __forceinline__ void hp_exchange(double (&d)[3], double (&V)[3][3]) {
    const bool s = d[B_] > d[A_];
    const double da = s ? d[B_] : d[A_], db = s ? d[A_] : d[B_];
    d[A_] = da, d[B_] = db;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double va = s ? V[i][B_] : V[i][A_], vb = s ? V[i][A_] : V[i][B_];
        V[i][A_] = va, V[i][B_] = vb;
    }
}

// Step 4 for one sign: u = (a*v1 + sb*v3) / c with sb = +b or -b (a*v1 - b*v3 and a*v1 + (-b)*v3 are the same operation).
// false: |T| is zero or not finite.
__device__ __forceinline__ bool hp_side(const double (&A)[9], const double (&v1)[3], const double (&v2)[3], const double (&v3)[3], double a, double sb,
                                        double c, double (&R)[9], double (&t)[3], double (&n)[3], double& invd) {
    double u[3], m1[3], m2[3], m3[3], An[3], Rn[3], T[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = (a * v1[i] + sb * v3[i]) / c;
    hp_mul(A, v2, m1);
    hp_mul(A, u, m2);
    hp_cross(m1, m2, m3);
    hp_cross(v2, u, n);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) R[3 * i + k] = (m1[i] * v2[k] + m2[i] * u[k]) + m3[i] * n[k];
    hp_mul(A, n, An);
    hp_mul(R, n, Rn);
#pragma unroll
    for (int i = 0; i < 3; ++i) T[i] = An[i] - Rn[i];
    invd = hp_norm(T);
    if (!g3_finite_nonzero(invd)) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = T[i] / invd;
    return true;
}

__device__ __forceinline__ bool hp_selected(const vslam_homography& m, int only_degenerate) {
    return m.best >= 0 && (!only_degenerate || m.degenerate != 0);
}

// grid = (pair blocks of 64), one lane per pair.  Writes info[j] (kind, spread, n_matches, ROTATION's R; the rest zero: the
// vote and the selection fill it), the four candidates and |T| of the two signs.
__global__ __launch_bounds__(HPOSE_PAIR_WG) void k_hpose_candidates(const vslam_homography* __restrict__ models, vslam_hpose_params P, int n_pairs,
                                                                     const unsigned int* __restrict__ counts, unsigned int mcap,
                                                                     vslam_hpose_cand* __restrict__ cand, double* __restrict__ invd,
                                                                     vslam_hpose* __restrict__ info) {
    const int j = blockIdx.x * HPOSE_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    double Rp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Rm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Rr[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double tp[3] = {0, 0, 0}, tm[3] = {0, 0, 0}, np_[3] = {0, 0, 0}, nm[3] = {0, 0, 0};
    double dp = 0.0, dm = 0.0, spread = 0.0;
    bool okp = false, okm = false;
    int kind = VSLAM_HPOSE_NONE;
    do {
        if (!hp_selected(models[j], P.only_degenerate)) break;
        // 1. A = K^-1 H K
        double G[9], A[9];
        const double* H = models[j].H;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            G[3 * i] = H[3 * i] * P.K.fx, G[3 * i + 1] = H[3 * i + 1] * P.K.fy;
            G[3 * i + 2] = (H[3 * i] * P.K.cx + H[3 * i + 1] * P.K.cy) + H[3 * i + 2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            A[c] = (G[c] - P.K.cx * G[6 + c]) / P.K.fx;
            A[3 + c] = (G[3 + c] - P.K.cy * G[6 + c]) / P.K.fy;
            A[6 + c] = G[6 + c];
        }
        // 2. eigenvalues of A^T A, brought into descending order by three exchanges; A scaled so that the middle one is 1
        double d[3], V[3][3];
        g3_gram_jacobi<6>(A, d, V);
        hp_exchange<0, 1>(d, V);
        hp_exchange<1, 2>(d, V);
        hp_exchange<0, 1>(d, V);
        const double L1 = d[0], L2 = d[1], L3 = d[2];
        if (!(L2 > 0.0) || !(L2 < __builtin_huge_val())) break;
        const double s = sqrt(L2);
#pragma unroll
        for (int i = 0; i < 9; ++i) A[i] = A[i] / s;
        const double l1 = L1 / L2, l3 = L3 / L2;
        const double sp = l1 - l3;
        // 3. the kind
        if (!(sp >= P.min_spread)) {
            double c1[3] = {A[0], A[3], A[6]}, c2[3] = {A[1], A[4], A[7]}, r1[3], r2[3], r3[3];
            const double n1 = hp_norm(c1);
            if (!g3_finite_nonzero(n1)) break;
#pragma unroll
            for (int i = 0; i < 3; ++i) r1[i] = c1[i] / n1;
            const double g = (r1[0] * c2[0] + r1[1] * c2[1]) + r1[2] * c2[2];
#pragma unroll
            for (int i = 0; i < 3; ++i) c2[i] = c2[i] - g * r1[i];
            const double n2 = hp_norm(c2);
            if (!g3_finite_nonzero(n2)) break;
#pragma unroll
            for (int i = 0; i < 3; ++i) r2[i] = c2[i] / n2;
            hp_cross(r1, r2, r3);
#pragma unroll
            for (int i = 0; i < 3; ++i) Rr[3 * i] = r1[i], Rr[3 * i + 1] = r2[i], Rr[3 * i + 2] = r3[i];
            spread = sp;
            kind = VSLAM_HPOSE_ROTATION;
            break;
        }
        // 4. the candidates of both signs
        const double v1[3] = {V[0][0], V[1][0], V[2][0]}, v2[3] = {V[0][1], V[1][1], V[2][1]}, v3[3] = {V[0][2], V[1][2], V[2][2]};
        const double a = sqrt(1.0 - l3), b = sqrt(l1 - 1.0), c = sqrt(sp);
        okp = hp_side(A, v1, v2, v3, a, b, c, Rp, tp, np_, dp);
        okm = hp_side(A, v1, v2, v3, a, -b, c, Rm, tm, nm, dm);
        spread = sp;
        kind = VSLAM_HPOSE_PLANE;
    } while (false);
    vslam_hpose_cand* out = cand + (size_t)j * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const bool ok = c < 2 ? okp : okm;
        const double sg = (c & 1) ? -1.0 : 1.0;  // (x * -1.0 is -x exactly)
#pragma unroll
        for (int i = 0; i < 9; ++i) out[c].R[i] = ok ? pose_canonical(c < 2 ? Rp[i] : Rm[i]) : 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            out[c].t[i] = ok ? pose_canonical(sg * (c < 2 ? tp[i] : tm[i])) : 0.0;
            out[c].n[i] = ok ? pose_canonical(sg * (c < 2 ? np_[i] : nm[i])) : 0.0;
        }
        out[c].front = 0;
        out[c].valid = ok ? 1 : 0;
    }
    invd[(size_t)j * 2] = okp ? dp : 0.0;
    invd[(size_t)j * 2 + 1] = okm ? dm : 0.0;
    vslam_hpose o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.R[i] = pose_canonical(Rr[i]);
    o.n[0] = o.n[1] = o.n[2] = 0.0;
    o.inv_d = 0.0;
    o.spread = pose_canonical(spread);
    o.n_matches = kind == VSLAM_HPOSE_NONE ? 0u : g3_count(counts, j, mcap);
    o.n_support = o.front = o.front_runner = 0;
    o.kind = kind;
    o.best = kind == VSLAM_HPOSE_NONE ? 0 : -1;
    o.ambiguous = o.resolved = 0;
    info[j] = o;
}

// The two votes of one sign: under (R, t, n) and under (R, -t, -n).
__device__ __forceinline__ void hp_votes(const vslam_hpose_cand& c, const PoseRays& r, bool sup, bool& fa, bool& fb) {
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = c.R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = c.t[k];
    double det, n1, n2;
    pose_solve(R, t, r, det, n1, n2);
    const double nq = (c.n[0] * r.q0 + c.n[1] * r.q1) + c.n[2];
    fa = sup && det > 0.0 && n1 > 0.0 && n2 > 0.0 && nq > 0.0;
    fb = sup && det > 0.0 && n1 < 0.0 && n2 < 0.0 && nq < 0.0;
}

// grid = (record blocks of 256, pairs).  The pair's H, G and candidates are read through addresses that are the same in
// every lane.  `cand` and `info` are read (R, t, n, valid; kind) and written (front, n_support, by atomicAdd) here, so they
// are neither const nor restrict.
__global__ __launch_bounds__(HPOSE_REC_WG) void k_hpose_vote(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                              const vslam_homography* __restrict__ models, vslam_pose_params K, double max_dist2,
                                                              vslam_hpose_cand* cand, vslam_hpose* info) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(counts, j, mcap);
    const size_t i = g3_record(blockIdx.x, HPOSE_REC_WG, threadIdx.x);
    if (!g3_wave_has_record(i, m)) return;
    const int kind = info[j].kind;
    if (kind == VSLAM_HPOSE_NONE) return;  // block-uniform: every count stays 0
    vslam_hpose_cand* cj = cand + (size_t)j * 4;
    bool sup = false, f0 = false, f1 = false, f2 = false, f3 = false;
    if (i < m) {
        const EpiXY p = xy[(size_t)j * mcap + i];
        double H[9], G[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) H[k] = models[j].H[k], G[k] = models[j].G[k];
        sup = hom_inlier(H, G, p, max_dist2);
        if (kind == VSLAM_HPOSE_PLANE) {
            const PoseRays r = pose_rays(p, K);
            if (cj[0].valid) hp_votes(cj[0], r, sup, f0, f1);
            if (cj[2].valid) hp_votes(cj[2], r, sup, f2, f3);
        }
    }
    const unsigned int cs = __popcll(__ballot(sup));
    const unsigned int c0 = __popcll(__ballot(f0)), c1 = __popcll(__ballot(f1)), c2 = __popcll(__ballot(f2)), c3 = __popcll(__ballot(f3));
    if (g3_first_lane(threadIdx.x)) {
        if (cs) atomicAdd(&info[j].n_support, cs);
        if (c0) atomicAdd(&cj[0].front, c0);
        if (c1) atomicAdd(&cj[1].front, c1);
        if (c2) atomicAdd(&cj[2].front, c2);
        if (c3) atomicAdd(&cj[3].front, c3);
    }
}

// grid = (pair blocks of 64), one lane per pair.  info[j] was begun by k_hpose_candidates and k_hpose_vote.
__global__ __launch_bounds__(HPOSE_PAIR_WG) void k_hpose_select(const vslam_homography* __restrict__ models, const vslam_hpose_cand* __restrict__ cand,
                                                                 const double* __restrict__ invd, const vslam_pose* __restrict__ priors,
                                                                 const unsigned int* __restrict__ counts, unsigned int mcap, int n_pairs,
                                                                 unsigned int num, unsigned int den, int only_degenerate, vslam_hpose* info,
                                                                 vslam_pose* __restrict__ poses) {
    const int j = blockIdx.x * HPOSE_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    if (!hp_selected(models[j], only_degenerate)) return;  // info[j] is the NONE record already, poses[j] stays
    const vslam_hpose_cand* cj = cand + (size_t)j * 4;
    const int kind = info[j].kind;
    int best = -1, w = -1;
    unsigned int most = 0, runner = 0;
    bool ambiguous = false, resolved = false;
    if (kind == VSLAM_HPOSE_PLANE) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (cj[c].front > most) most = cj[c].front, w = c;  // strictly more: the lowest c on ties, and a count of 0 never wins
        best = w;
        if (w >= 0) {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c != w && cj[c].front > runner) runner = cj[c].front;
            ambiguous = (unsigned long long)runner * den >= (unsigned long long)num * most;
            if (ambiguous && priors && priors[j].best >= 0) {
                resolved = true;
                double kept = 0.0;
                bool have = false;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (!((unsigned long long)cj[c].front * den >= (unsigned long long)num * most)) continue;
                    if (!cj[c].valid) continue;  // (a candidate that is not valid has front 0: only num == 0 brings it here)
                    double s = priors[j].R[0] * cj[c].R[0];
#pragma unroll
                    for (int k = 1; k < 9; ++k) s = s + priors[j].R[k] * cj[c].R[k];
                    if (!have || s > kept) kept = s, best = c, have = true;
                }
            }
        }
    }
    const bool carry = best >= 0 && (!ambiguous || resolved);
    vslam_pose out;
#pragma unroll
    for (int i = 0; i < 9; ++i) out.R[i] = carry ? cj[best].R[i] : 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) out.t[i] = carry ? cj[best].t[i] : 0.0;
    out.n_matches = g3_count(counts, j, mcap);
    out.n_front = carry ? cj[best].front : 0u;
    out.best = carry ? best : -1;
    out.valid = kind == VSLAM_HPOSE_PLANE ? 1 : 0;
    poses[j] = out;
    if (kind == VSLAM_HPOSE_PLANE && best >= 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) info[j].R[i] = cj[best].R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) info[j].n[i] = cj[best].n[i];
        info[j].inv_d = best < 2 ? invd[(size_t)j * 2] : invd[(size_t)j * 2 + 1];
        info[j].front = most;
        info[j].front_runner = runner;
        info[j].best = best;
        info[j].ambiguous = ambiguous ? 1 : 0;
        info[j].resolved = resolved ? 1 : 0;
    }
}

// grid = (record blocks of 256, pairs), selected pairs only: X of every record below the count (points may be null), and bit
// i % 64 of word i / 64 = record i is supported and in front under poses[j] (bits may be null).  Without a pose the words are
// zero and no point is written.
__global__ __launch_bounds__(HPOSE_REC_WG) void k_hpose_points(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                                const vslam_homography* __restrict__ models, const vslam_pose* __restrict__ poses,
                                                                vslam_pose_params K, double max_dist2, int only_degenerate,
                                                                double* __restrict__ points, unsigned long long* __restrict__ bits, unsigned int fwords) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(counts, j, mcap);
    const size_t i = g3_record(blockIdx.x, HPOSE_REC_WG, threadIdx.x);
    if (!g3_wave_has_record(i, m)) return;
    if (!hp_selected(models[j], only_degenerate)) return;  // block-uniform: the pair's rows and words stay as they are
    const bool lane0 = g3_first_lane(threadIdx.x);
    if (poses[j].best < 0) {  // block-uniform
        g3_store_word(bits, j, fwords, i, bits && lane0, 0ull);
        return;
    }
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = poses[j].R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = poses[j].t[k];
    bool in = false;
    if (i < m) {
        const EpiXY p = xy[(size_t)j * mcap + i];
        double H[9], G[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) H[k] = models[j].H[k], G[k] = models[j].G[k];
        const bool sup = hom_inlier(H, G, p, max_dist2);
        const PoseRays r = pose_rays(p, K);
        double det, n1, n2;
        pose_solve(R, t, r, det, n1, n2);
        in = sup && det > 0.0 && n1 > 0.0 && n2 > 0.0;
        if (points) {
            const double l1 = n1 / det, l2 = n2 / det;
            const double c0 = l2 * r.b0 - t[0], c1 = l2 * r.b1 - t[1], c2 = l2 - t[2];
            const double P0 = (R[0] * c0 + R[3] * c1) + R[6] * c2, P1 = (R[1] * c0 + R[4] * c1) + R[7] * c2, P2 = (R[2] * c0 + R[5] * c1) + R[8] * c2;
            const double nan = __longlong_as_double(0x7ff8000000000000ll);
            double* X = points + ((size_t)j * mcap + i) * 3;
            X[0] = sup ? pose_canonical(0.5 * (l1 * r.q0 + P0)) : nan;
            X[1] = sup ? pose_canonical(0.5 * (l1 * r.q1 + P1)) : nan;
            X[2] = sup ? pose_canonical(0.5 * (l1 + P2)) : nan;
        }
    }
    const unsigned long long w = __ballot(in);
    g3_store_word(bits, j, fwords, i, bits && lane0, w);
}

}  // namespace vslam
