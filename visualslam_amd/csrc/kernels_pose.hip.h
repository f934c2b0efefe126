// Relative pose and triangulation (include/vslam.h, "relative pose and triangulation"): from the fundamental matrix of every
// pair and a match list to (R, t) and the 3-D point of every record.
//   k_pose_candidates : one lane per pair: E = K^T F K, its singular vectors by the Jacobi sweeps of the two-view model, the
//                       four (R, t) candidates (steps 1 - 4); everything in registers, statically indexed
//   k_pose_vote       : the hot path, one lane per match record: the cheirality test under both rotations - the sign of t
//                       flips n1 and n2 exactly, so two evaluations give all four votes; ballot + popcount per wave, one
//                       integer atomicAdd per wave and candidate
//   k_pose_select     : one lane per pair: the candidate with the most records in front, lowest index on ties
//   k_pose_points     : one lane per record: the midpoint of the two rays under the winner, and the wave's ballot word
// The {x, y, x', y'} records come from k_epi_coords (vslam::enqueue_epi_coords).  The arithmetic is the header's, operation
// for operation, under the rules of kernels_epipolar.hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_geom3.hip.h"
#include "vslam_pose_plan.h"

namespace vslam {

__device__ __forceinline__ void pose_cross(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// w = E v, then u = w / |w|; false: the norm is zero or not finite.  `u1`: w is first made orthogonal to it (step 3's w2).
__device__ __forceinline__ bool pose_left_vector(const double (&E)[9], const double (&v)[3], const double* u1, double (&u)[3]) {
    double w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = (E[3 * i] * v[0] + E[3 * i + 1] * v[1]) + E[3 * i + 2] * v[2];
    if (u1) {
        const double d = (u1[0] * w[0] + u1[1] * w[1]) + u1[2] * w[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) w[i] = w[i] - d * u1[i];
    }
    const double n = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    if (!g3_finite_nonzero(n)) return false;
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = w[i] / n;
    return true;
}

// grid = (pair blocks of 64), one lane per pair.
__global__ __launch_bounds__(POSE_PAIR_WG) void k_pose_candidates(const vslam_epipolar* __restrict__ models, vslam_pose_params K, int n_pairs,
                                                                   vslam_pose_cand* __restrict__ cand) {
    const int j = blockIdx.x * POSE_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    double Ra[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Rb[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, u3[3] = {0, 0, 0};
    bool ok = false;
    do {
        if (models[j].best < 0) break;
        // 1. E = K^T F K, Frobenius norm 1
        double E[9];
        const G3Affine Km{K.fx, K.fy, K.cx, K.cy};
        g3_lt_f_r(Km, models[j].F, Km, E);
        const double nrm = g3_frobenius(E);
        if (!g3_finite_nonzero(nrm)) break;
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] = E[i] / nrm;
        // 2. right singular vectors: cyclic Jacobi on S = E^T E
        double S[3], V[3][3];
        g3_gram_jacobi<6>(E, S, V);
        int k = 0;
        double smin = S[0];
        if (S[1] < smin) k = 1, smin = S[1];
        if (S[2] < smin) k = 2, smin = S[2];
        // (p, q) = (1, 2), (0, 2), (0, 1) for k = 0, 1, 2: selects, not indexed reads
        double v1[3], v2[3], v3[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            v1[i] = k == 0 ? V[i][1] : V[i][0];
            v2[i] = k == 2 ? V[i][1] : V[i][2];
        }
        pose_cross(v1, v2, v3);
        // 3. left singular vectors
        double u1[3], u2[3];
        if (!pose_left_vector(E, v1, nullptr, u1)) break;
        if (!pose_left_vector(E, v2, u1, u2)) break;
        pose_cross(u1, u2, u3);
        // 4. the two rotations
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Ra[3 * i + c] = (u2[i] * v1[c] - u1[i] * v2[c]) + u3[i] * v3[c];
                Rb[3 * i + c] = (u1[i] * v2[c] - u2[i] * v1[c]) + u3[i] * v3[c];
            }
        ok = true;
    } while (false);
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 9; ++i) Ra[i] = Rb[i] = 0.0;
        u3[0] = u3[1] = u3[2] = 0.0;
    }
    vslam_pose_cand* out = cand + (size_t)j * 4;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int i = 0; i < 9; ++i) out[c].R[i] = c < 2 ? Ra[i] : Rb[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) out[c].t[i] = (c & 1) && ok ? -u3[i] : u3[i];
        out[c].front = 0;
        out[c].valid = ok ? 1 : 0;
    }
}

// grid = (record blocks of 256, pairs).  The pair's candidates are read through addresses that are the same in every lane.
// `cand` is read (R, t, valid) and written (front, by atomicAdd) here, so it is neither const nor restrict.
__global__ __launch_bounds__(POSE_REC_WG) void k_pose_vote(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts,
                                                            unsigned int mcap, vslam_pose_params K, vslam_pose_cand* cand) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(counts, j, mcap);
    const size_t i = g3_record(blockIdx.x, POSE_REC_WG, threadIdx.x);
    if (!g3_wave_has_record(i, m)) return;
    vslam_pose_cand* cj = cand + (size_t)j * 4;
    if (!cj[0].valid) return;  // block-uniform: every count stays 0
    double Ra[9], Rb[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Ra[k] = cj[0].R[k], Rb[k] = cj[2].R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = cj[0].t[k];
    bool f0 = false, f1 = false, f2 = false, f3 = false;
    if (i < m) {
        const PoseRays r = pose_rays(xy[(size_t)j * mcap + i], K);
        double det, n1, n2;
        pose_solve(Ra, t, r, det, n1, n2);
        f0 = det > 0.0 && n1 > 0.0 && n2 > 0.0;
        f1 = det > 0.0 && n1 < 0.0 && n2 < 0.0;  // under -t: -n1 > 0 && -n2 > 0
        pose_solve(Rb, t, r, det, n1, n2);
        f2 = det > 0.0 && n1 > 0.0 && n2 > 0.0;
        f3 = det > 0.0 && n1 < 0.0 && n2 < 0.0;
    }
    const unsigned int c0 = __popcll(__ballot(f0)), c1 = __popcll(__ballot(f1)), c2 = __popcll(__ballot(f2)), c3 = __popcll(__ballot(f3));
    if (g3_first_lane(threadIdx.x)) {
        if (c0) atomicAdd(&cj[0].front, c0);
        if (c1) atomicAdd(&cj[1].front, c1);
        if (c2) atomicAdd(&cj[2].front, c2);
        if (c3) atomicAdd(&cj[3].front, c3);
    }
}

// grid = (pair blocks of 64), one lane per pair.
__global__ __launch_bounds__(POSE_PAIR_WG) void k_pose_select(const vslam_pose_cand* __restrict__ cand, const unsigned int* __restrict__ counts,
                                                               unsigned int mcap, int n_pairs, vslam_pose* __restrict__ poses) {
    const int j = blockIdx.x * POSE_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    const vslam_pose_cand* cj = cand + (size_t)j * 4;
    int best = -1;
    unsigned int most = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
        if (cj[c].front > most) most = cj[c].front, best = c;  // strictly more: the lowest c on ties, and a count of 0 never wins
    const int valid = cj[0].valid;
    if (!valid) best = -1;
    vslam_pose out;
#pragma unroll
    for (int i = 0; i < 9; ++i) out.R[i] = best < 0 ? 0.0 : cj[best].R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) out.t[i] = best < 0 ? 0.0 : cj[best].t[i];
    out.n_matches = g3_count(counts, j, mcap);
    out.n_front = best < 0 ? 0u : most;
    out.best = best;
    out.valid = valid;
    poses[j] = out;
}

// grid = (record blocks of 256, pairs): X of every record below the count (points may be null), and bit i % 64 of word i / 64
// = record i is in front under the winner (bits may be null).  Without a winner the words are zero and no point is written.
__global__ __launch_bounds__(POSE_REC_WG) void k_pose_points(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts,
                                                              unsigned int mcap, const vslam_pose* __restrict__ poses, vslam_pose_params K,
                                                              double* __restrict__ points, unsigned long long* __restrict__ bits, unsigned int fwords) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(counts, j, mcap);
    const size_t i = g3_record(blockIdx.x, POSE_REC_WG, threadIdx.x);
    if (!g3_wave_has_record(i, m)) return;
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
        const PoseRays r = pose_rays(xy[(size_t)j * mcap + i], K);
        double det, n1, n2;
        pose_solve(R, t, r, det, n1, n2);
        in = det > 0.0 && n1 > 0.0 && n2 > 0.0;
        if (points) {
            const double l1 = n1 / det, l2 = n2 / det;
            const double c0 = l2 * r.b0 - t[0], c1 = l2 * r.b1 - t[1], c2 = l2 - t[2];
            const double P0 = (R[0] * c0 + R[3] * c1) + R[6] * c2, P1 = (R[1] * c0 + R[4] * c1) + R[7] * c2, P2 = (R[2] * c0 + R[5] * c1) + R[8] * c2;
            double* X = points + ((size_t)j * mcap + i) * 3;
            X[0] = pose_canonical(0.5 * (l1 * r.q0 + P0));
            X[1] = pose_canonical(0.5 * (l1 * r.q1 + P1));
            X[2] = pose_canonical(0.5 * (l1 + P2));
        }
    }
    const unsigned long long w = __ballot(in);
    g3_store_word(bits, j, fwords, i, bits && lane0, w);
}

}  // namespace vslam
