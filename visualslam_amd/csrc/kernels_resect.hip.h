// Resection (include/vslam.h, "resection"): the camera of frame j + 1 from the points pair j - 1 triangulated and their
// observations in frame j + 1, by RANSAC over a calibrated 6-point DLT.
//   k_res_corr   : one lane per observation record: the link a = prev[j][query] (the table is k_chain_link's), step 2's Y, u, v,
//                  the wave's ballot word of usable records, {b, a} for the compaction (kernels_compact.hip.h, EpipolarEntries)
//   k_res_gather : one lane per row of the dense list: {b, a} -> {Y, u, v, b}, step 2 again from the same inputs
//   k_res_models : one lane per (pair, hypothesis): sample 6 correspondences, the 12 x 12 Gauss-Jordan in LDS, M and m, the
//                  rotation nearest to M by the pose section's Jacobi sweeps, t = m / lambda
//   k_res_score  : the hot path, pairs x hypotheses x correspondences reprojection tests: one lane per hypothesis with R, t and
//                  the focal lengths in registers, the workgroup walks correspondence tiles staged in LDS (every lane reads the
//                  same address: a broadcast); 17 multiplications and 12 additions per test
//   k_res_select : one workgroup per pair: the valid hypothesis with the most inliers, lowest index on ties
//   k_res_flags  : one lane per observation record: usable and an inlier of the winner, the wave's ballot word
// Kernel boundaries order everything: no flags or fences between workgroups, no floating-point atomics.  The arithmetic is the
// header's, operation for operation, under the rules of kernels_epipolar.hip.h.  The Gauss-Jordan loop is written out again, as
// in kernels_homography.hip.h: the sizes differ, and the existing kernels' allocation must not move.  k_res_select is the shared
// RANSAC step of kernels_estimate.hip.h; k_res_score keeps its own text, as k_epi_score does, and k_res_flags recomputes the
// correspondence and stays here.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_estimate.hip.h"
#include "kernels_geom3.hip.h"
#include "vslam_resect_plan.h"

namespace vslam {

constexpr unsigned int RES_NO_LINK = 0xffffffffu;  // a link-table entry no live record wrote (k_chain_link's table)

// What the record kernels need to know of one call's inputs.
struct ResIn {
    const vslam_pose* poses;
    const double* points;
    unsigned int mcap, pcap;  // the structure side's match capacity (the row pitch of points), and point_cap
    const vslam_match* obs;
    const unsigned int* ocounts;
    unsigned int ocap;
    const vslam_point* tpts;
    unsigned int tcap;
    vslam_pose_params K;
};

__device__ __forceinline__ bool res_finite(double x) { return fabs(x) < __builtin_huge_val(); }

// Step 2 of record (train index `train`, link a) of pair j >= 1: candidate, then Y, u, v; true: usable.
__device__ __forceinline__ bool res_correspondence(const ResIn& in, int j, unsigned int train, int a, ResYuv& o) {
    if (a < 0 || train >= in.tcap) return false;
    const vslam_point t = in.tpts[(size_t)j * in.tcap + train];
    if ((unsigned int)t.octave > 31u) return false;
    const double st = t.octave == 0 ? 0.5 : (double)(1u << (t.octave - 1));
    const double xp = (double)((long long)t.col - (long long)t.padding) * st;
    const double yp = (double)((long long)t.row - (long long)t.padding) * st;
    o.u = (xp - in.K.cx) / in.K.fx;
    o.v = (yp - in.K.cy) / in.K.fy;
    const vslam_pose& P = in.poses[j - 1];
    const double* X = in.points + ((size_t)(j - 1) * in.mcap + (unsigned int)a) * 3;
    const double X0 = X[0], X1 = X[1], X2 = X[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) o.Y[i] = ((P.R[3 * i] * X0 + P.R[3 * i + 1] * X1) + P.R[3 * i + 2] * X2) + P.t[i];
    return res_finite(o.Y[0]) && res_finite(o.Y[1]) && res_finite(o.Y[2]);
}

// grid = (record blocks of 256, n_pairs).  prev [n_pairs - 1][pcap] has no row for pair 0, which has no links.  idx [n_pairs][ocap]
// gets {query = b, train = a}; uflags the ballot words that hold a record below the count; links may be null.
__global__ __launch_bounds__(TWOVIEW_REC_WG) void k_res_corr(ResIn in, const unsigned int* __restrict__ prev, vslam_match* __restrict__ idx,
                                                              unsigned long long* __restrict__ uflags, unsigned int fwords, int* __restrict__ links) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(in.ocounts, j, in.ocap);
    const size_t b = g3_record(blockIdx.x, TWOVIEW_REC_WG, threadIdx.x);
    if (!g3_wave_has_record(b, m)) return;
    bool use = false;
    if (b < m) {
        const size_t o = (size_t)j * in.ocap + b;
        const vslam_match rec = in.obs[o];
        int a = -1;
        if (j >= 1 && (unsigned int)rec.query < in.pcap) {
            const unsigned int p = prev[(size_t)(j - 1) * in.pcap + (unsigned int)rec.query];
            if (p != RES_NO_LINK) a = (int)p;
        }
        ResYuv c;
        use = res_correspondence(in, j, (unsigned int)rec.train, a, c);
        vslam_match e;
        e.query = (int)b, e.train = a, e.dist2 = 0.0f;
        idx[o] = e;
        if (links) links[o] = a;
    }
    const unsigned long long w = __ballot(use);
    g3_store_word(uflags, j, fwords, b, g3_first_lane(threadIdx.x), w);
}

// grid = (record blocks of 256, n_pairs).  didx [n_pairs][ocap]: the compacted {b, a}; ncorr [n_pairs] their counts.
__global__ __launch_bounds__(TWOVIEW_REC_WG) void k_res_gather(ResIn in, const vslam_match* __restrict__ didx, const unsigned int* __restrict__ ncorr,
                                                                vslam_resect_corr* __restrict__ corr) {
    const int j = blockIdx.y;
    const unsigned int n = g3_count(ncorr, j, in.ocap);
    const size_t r = g3_record(blockIdx.x, TWOVIEW_REC_WG, threadIdx.x);
    if (r >= n) return;
    const vslam_match e = didx[(size_t)j * in.ocap + r];
    ResYuv c;
    (void)res_correspondence(in, j, (unsigned int)in.obs[(size_t)j * in.ocap + (unsigned int)e.query].train, e.train, c);
    vslam_resect_corr out;
    out.Y[0] = c.Y[0], out.Y[1] = c.Y[1], out.Y[2] = c.Y[2], out.u = c.u, out.v = c.v;
    out.b = (unsigned int)e.query, out.reserved = 0;
    corr[(size_t)j * in.ocap + r] = out;
}

__device__ __forceinline__ void res_cross(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ void res_mul(const double (&M)[9], const double (&v)[3], double (&w)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = (M[3 * i] * v[0] + M[3 * i + 1] * v[1]) + M[3 * i + 2] * v[2];
}
__device__ __forceinline__ double res_norm(const double (&w)[3]) { return sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]); }

// The inlier test of one correspondence under (R, t) (step 6); false for R = t = 0 (Z2 > 0 fails).
__device__ __forceinline__ bool res_inlier(const double (&R)[9], const double (&t)[3], double fx, double fy, const ResYuv& c, double max_dist2) {
    const double Z0 = ((R[0] * c.Y[0] + R[1] * c.Y[1]) + R[2] * c.Y[2]) + t[0];
    const double Z1 = ((R[3] * c.Y[0] + R[4] * c.Y[1]) + R[5] * c.Y[2]) + t[1];
    const double Z2 = ((R[6] * c.Y[0] + R[7] * c.Y[1]) + R[8] * c.Y[2]) + t[2];
    const double ex = (c.u * Z2 - Z0) * fx, ey = (c.v * Z2 - Z1) * fy;
    return Z2 > 0.0 && (ex * ex + ey * ey) < max_dist2 * (Z2 * Z2);
}

// grid = (hypothesis blocks of 64, pairs), one wave.  The 12 x 12 matrix is indexed by a data-dependent pivot, so it lives in
// LDS, lane-strided: element e of lane l at a[e][l] - the 64 lanes of one access hit 64 consecutive f64, no bank conflict.
// 73728 + 1536 bytes of LDS: two workgroups per compute unit.  The six sample points stay in registers, statically indexed.
__global__ __launch_bounds__(RES_MODEL_WG) void k_res_models(const vslam_resect_corr* __restrict__ corr, const unsigned int* __restrict__ ncorr,
                                                              unsigned int ocap, unsigned int NH, unsigned int seed,
                                                              vslam_resect_hyp* __restrict__ hyp) {
    __shared__ double a[144][RES_MODEL_WG];
    __shared__ unsigned int sidx[6][RES_MODEL_WG];
    const int j = blockIdx.y, l = threadIdx.x;
    const unsigned int h = blockIdx.x * RES_MODEL_WG + l;
    if (h >= NH) return;  // (no barrier below: every lane works on its own columns of the arrays)
    vslam_resect_hyp* out = hyp + (size_t)j * NH + h;
    double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t[3] = {0, 0, 0};
    bool ok = false;
    const unsigned int m = g3_count(ncorr, j, ocap);
    do {
        if (m < 6) break;
        // 3. the sample
        const unsigned int base = epi_mix(epi_mix(seed + (unsigned int)j) + h);
        int n = 0;
        for (unsigned int d = 0; d < 64 && n < 6; ++d) {
            const unsigned int r = epi_mix(base + d);
            const unsigned int i = (unsigned int)(((unsigned long long)r * m) >> 32);
            bool seen = false;
            for (int k = 0; k < n; ++k) seen |= sidx[k][l] == i;
            if (!seen) sidx[n++][l] = i;
        }
        if (n < 6) break;
        double Y[6][3], u[6], v[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const vslam_resect_corr& c = corr[(size_t)j * ocap + sidx[i][l]];
            Y[i][0] = c.Y[0], Y[i][1] = c.Y[1], Y[i][2] = c.Y[2], u[i] = c.u, v[i] = c.v;
        }
        // 4a. normalise the six points
        double cen[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) cen[k] = (((((Y[0][k] + Y[1][k]) + Y[2][k]) + Y[3][k]) + Y[4][k]) + Y[5][k]) / 6.0;
        double dsum = 0.0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double e0 = Y[i][0] - cen[0], e1 = Y[i][1] - cen[1], e2 = Y[i][2] - cen[2];
            const double r = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
            dsum = i == 0 ? r : dsum + r;
        }
        const double dm = dsum / 6.0;
        if (dm == 0.0) break;
        const double s = 1.7320508075688772 / dm;
        // 4b. the 12 x 12 matrix
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double N0 = (Y[i][0] - cen[0]) * s, N1 = (Y[i][1] - cen[1]) * s, N2 = (Y[i][2] - cen[2]) * s;
            const int r0 = 24 * i, r1 = 24 * i + 12;
            a[r0 + 0][l] = N0, a[r0 + 1][l] = N1, a[r0 + 2][l] = N2, a[r0 + 3][l] = 1.0;
            a[r0 + 4][l] = 0.0, a[r0 + 5][l] = 0.0, a[r0 + 6][l] = 0.0, a[r0 + 7][l] = 0.0;
            a[r0 + 8][l] = -(u[i] * N0), a[r0 + 9][l] = -(u[i] * N1), a[r0 + 10][l] = -(u[i] * N2), a[r0 + 11][l] = -u[i];
            a[r1 + 0][l] = 0.0, a[r1 + 1][l] = 0.0, a[r1 + 2][l] = 0.0, a[r1 + 3][l] = 0.0;
            a[r1 + 4][l] = N0, a[r1 + 5][l] = N1, a[r1 + 6][l] = N2, a[r1 + 7][l] = 1.0;
            a[r1 + 8][l] = -(v[i] * N0), a[r1 + 9][l] = -(v[i] * N1), a[r1 + 10][l] = -(v[i] * N2), a[r1 + 11][l] = -v[i];
        }
        // 4c. Gauss-Jordan, full pivoting
        unsigned int used = 0;
        unsigned long long pcs = 0;  // chosen columns: bit mask, and 4 bits per step
        bool solved = true;
        for (int k = 0; k < 11; ++k) {
            double best = 0.0;
            int pr = -1, pc = -1;
            for (int r = k; r < 12; ++r)
                for (int c = 0; c < 12; ++c) {
                    if (used >> c & 1u) continue;
                    const double x = fabs(a[12 * r + c][l]);
                    if (x > best) best = x, pr = r, pc = c;
                }
            if (pr < 0 || !(best < __builtin_huge_val())) {
                solved = false;
                break;
            }
            if (pr != k)
                for (int c = 0; c < 12; ++c) {
                    const double x = a[12 * k + c][l];
                    a[12 * k + c][l] = a[12 * pr + c][l];
                    a[12 * pr + c][l] = x;
                }
            const double p = a[12 * k + pc][l];
            double rowk[12];
#pragma unroll
            for (int c = 0; c < 12; ++c) {
                rowk[c] = a[12 * k + c][l] / p;
                a[12 * k + c][l] = rowk[c];
            }
            for (int r = 0; r < 12; ++r) {
                if (r == k) continue;
                const double g = a[12 * r + pc][l];
#pragma unroll
                for (int c = 0; c < 12; ++c) a[12 * r + c][l] = a[12 * r + c][l] - g * rowk[c];
            }
            used |= 1u << pc;
            pcs |= (unsigned long long)pc << (4 * k);
        }
        if (!solved) break;
        const int fr = __ffs((int)(~used & 0xfffu)) - 1;
        // p lives in row 0's slots from here on (the matrix is no longer needed once the free column is read out)
        double fk[11];
#pragma unroll
        for (int k = 0; k < 11; ++k) fk[k] = -a[12 * k + fr][l];
        a[fr][l] = 1.0;
#pragma unroll
        for (int k = 0; k < 11; ++k) a[(unsigned int)(pcs >> (4 * k)) & 15u][l] = fk[k];
        double p[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) p[i] = a[i][l];
        // 4d. undo the normalisation
        double M[9], mv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            M[3 * i] = p[4 * i] * s, M[3 * i + 1] = p[4 * i + 1] * s, M[3 * i + 2] = p[4 * i + 2] * s;
            mv[i] = p[4 * i + 3] - ((M[3 * i] * cen[0] + M[3 * i + 1] * cen[1]) + M[3 * i + 2] * cen[2]);
        }
        // 4e. the sign: det(M) > 0
        const double det = (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
        if (!g3_finite_nonzero(fabs(det))) break;
        if (det < 0.0) {
#pragma unroll
            for (int i = 0; i < 9; ++i) M[i] = -M[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) mv[i] = -mv[i];
        }
        // 5. the rotation nearest to M, and the scale
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
        res_cross(v1, v2, v3);
        double w1[3], w2[3], w3[3], u1[3], u2[3], u3[3];
        res_mul(M, v1, w1);
        const double n1 = res_norm(w1);
        if (!g3_finite_nonzero(n1)) break;
#pragma unroll
        for (int i = 0; i < 3; ++i) u1[i] = w1[i] / n1;
        res_mul(M, v2, w2);
        const double g = (u1[0] * w2[0] + u1[1] * w2[1]) + u1[2] * w2[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) w2[i] = w2[i] - g * u1[i];
        const double n2 = res_norm(w2);
        if (!g3_finite_nonzero(n2)) break;
#pragma unroll
        for (int i = 0; i < 3; ++i) u2[i] = w2[i] / n2;
        res_cross(u1, u2, u3);
        res_mul(M, v3, w3);
        const double n3 = res_norm(w3);
        const double lam = ((n1 + n2) + n3) / 3.0;
        if (!g3_finite_nonzero(lam)) break;
        double Rc[9], tc[3];
        bool fin = true;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                Rc[3 * i + c] = (u1[i] * v1[c] + u2[i] * v2[c]) + u3[i] * v3[c];
                fin &= res_finite(Rc[3 * i + c]);
            }
            tc[i] = mv[i] / lam;
            fin &= res_finite(tc[i]);
        }
        if (!fin) break;
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Rc[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = tc[i];
        ok = true;
    } while (false);
#pragma unroll
    for (int i = 0; i < 9; ++i) out->R[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) out->t[i] = t[i];
    out->inliers = 0;
    out->valid = ok ? 1 : 0;
}

// grid = (hypothesis blocks of 256, nsplit, pairs).  Lane = hypothesis; the workgroup's correspondence tiles (tile index =
// blockIdx.y + k * nsplit) are staged in LDS and every lane walks them in step: the LDS address is the same in all lanes.  The
// lane's integer count goes into its hypothesis by atomicAdd: integer sums merge exactly in any order.
__global__ __launch_bounds__(EPI_SCORE_WG) void k_res_score(const vslam_resect_corr* __restrict__ corr, const unsigned int* __restrict__ ncorr,
                                                             unsigned int ocap, unsigned int NH, double fx, double fy, double max_dist2,
                                                             vslam_resect_hyp* __restrict__ hyp) {
    __shared__ ResYuv tile[EPI_TILE];
    const int j = blockIdx.z;
    const unsigned int m = g3_count(ncorr, j, ocap);
    const unsigned int h = blockIdx.x * EPI_SCORE_WG + threadIdx.x;
    vslam_resect_hyp* mine = hyp + (size_t)j * NH + min(h, NH - 1);
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = mine->R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = mine->t[i];
    const vslam_resect_corr* src = corr + (size_t)j * ocap;
    unsigned int count = 0;
    for (size_t t0 = (size_t)blockIdx.y * EPI_TILE; t0 < m; t0 += (size_t)gridDim.y * EPI_TILE) {  // block-uniform trip count
        const unsigned int n = (unsigned int)min((size_t)EPI_TILE, m - t0);
        __syncthreads();
        static_assert(EPI_TILE == EPI_SCORE_WG, "one correspondence per lane when a tile is staged");
        if (threadIdx.x < n) {
            const vslam_resect_corr& c = src[t0 + threadIdx.x];
            tile[threadIdx.x] = ResYuv{{c.Y[0], c.Y[1], c.Y[2]}, c.u, c.v};
        }
        __syncthreads();
        if (n == EPI_TILE) {
#pragma unroll 4
            for (unsigned int i = 0; i < EPI_TILE; ++i) count += res_inlier(R, t, fx, fy, tile[i], max_dist2) ? 1u : 0u;
        } else {
            for (unsigned int i = 0; i < n; ++i) count += res_inlier(R, t, fx, fy, tile[i], max_dist2) ? 1u : 0u;
        }
    }
    if (h < NH && count) atomicAdd(&mine->inliers, count);
}

// grid = (pairs)
__global__ __launch_bounds__(256) void k_res_select(const vslam_resect_hyp* __restrict__ hyp, const unsigned int* __restrict__ ocounts,
                                                     unsigned int ocap, const unsigned int* __restrict__ ncorr, unsigned int NH,
                                                     vslam_resect* __restrict__ models) {
    const int j = blockIdx.x;
    ransac_select<ResModel>(hyp + (size_t)j * NH, NH, models + j, [&](vslam_resect& out) {
        out.n_obs = g3_count(ocounts, j, ocap);
        out.n_corr = g3_count(ncorr, j, ocap);
        out.reserved = 0;
    });
}

// grid = (record blocks of 256, pairs): bit b % 64 of word b / 64 = observation record b is usable and an inlier of the winner;
// the words that hold a record below the count are written (all zero without a winner: R = t = 0), the others left alone.
__global__ __launch_bounds__(TWOVIEW_REC_WG) void k_res_flags(ResIn in, const vslam_match* __restrict__ idx, const vslam_resect* __restrict__ models,
                                                               double max_dist2, unsigned long long* __restrict__ flags, unsigned int fwords) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(in.ocounts, j, in.ocap);
    const size_t b = g3_record(blockIdx.x, TWOVIEW_REC_WG, threadIdx.x);
    if (!g3_wave_has_record(b, m)) return;
    bool inl = false;
    if (b < m && models[j].best >= 0) {
        const size_t o = (size_t)j * in.ocap + b;
        ResYuv c;
        if (res_correspondence(in, j, (unsigned int)in.obs[o].train, idx[o].train, c)) {
            double R[9], t[3];
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = models[j].R[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = models[j].t[i];
            inl = res_inlier(R, t, in.K.fx, in.K.fy, c, max_dist2);
        }
    }
    const unsigned long long w = __ballot(inl);
    g3_store_word(flags, j, fwords, b, g3_first_lane(threadIdx.x), w);
}

}  // namespace vslam
