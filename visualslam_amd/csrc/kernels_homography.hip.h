// Homography and the degeneracy verdict (include/vslam.h, "homography and the degeneracy verdict"): RANSAC homography of
// every pair of a batch, beside the fundamental matrix, and the integer verdict that gates F where H explains the matches.
//   k_hom_models  : one lane per (pair, hypothesis): sample 4 records, normalised DLT, H with its sign, G = adj(H)
//   k_hom_score   : the hot path, pairs x hypotheses x records symmetric-transfer tests: one lane per hypothesis with H and G
//                   in registers, the workgroup walks record tiles staged in LDS (every lane reads the same address)
//   k_hom_select  : one workgroup per pair: the valid hypothesis with the most inliers, lowest index on ties
//   k_hom_flags   : the winner's inlier ballot words; kernels_compact.hip.h (EpipolarEntries) turns them into the list
//   k_hom_verdict : one lane per pair: n_epipolar, degenerate, and the gated copy of the epipolar model
// k_hom_select and k_hom_flags are the shared RANSAC steps of kernels_estimate.hip.h under this stage's model; k_hom_score keeps
// its own text, as k_epi_score does.  The coordinate scratch is k_epi_coords' (vslam::enqueue_epi_coords).  The arithmetic is
// the header's, operation for operation, as in kernels_epipolar.hip.h.  What is NOT shared with k_epi_models, on purpose: the normalisation over 4 points
// and the Gauss-Jordan loop are written out again here - k_epi_models stands at its register and scratch budget
// (kernels_geom3.hip.h), and routing its lines through a shared function is what changed its allocation before.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_estimate.hip.h"
#include "kernels_geom3.hip.h"
#include "vslam_homography_plan.h"

namespace vslam {

// Step 1 of the model for one side: the 4 values are read through `get(i)`.
template <class GetX, class GetY>
__device__ __forceinline__ bool hom_normalise(GetX gx, GetY gy, double& cx, double& cy, double& s) {
    cx = (((gx(0) + gx(1)) + gx(2)) + gx(3)) / 4.0;
    cy = (((gy(0) + gy(1)) + gy(2)) + gy(3)) / 4.0;
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double dx = gx(i) - cx, dy = gy(i) - cy;
        const double r = sqrt(dx * dx + dy * dy);
        d = i == 0 ? r : d + r;
    }
    d = d / 4.0;
    if (d == 0.0) return false;
    s = 1.4142135623730951 / d;
    return true;
}

// grid = (hypothesis blocks of 64, pairs), one wave.  The 8 x 9 matrix is indexed by a data-dependent pivot, so it lives in
// LDS, lane-strided: element e of lane l at a[e][l] - the 64 lanes of one access hit 64 consecutive f64, no bank conflict.
__global__ __launch_bounds__(HOM_MODEL_WG) void k_hom_models(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts,
                                                              unsigned int mcap, unsigned int NH, unsigned int seed,
                                                              vslam_homography_hyp* __restrict__ hyp) {
    __shared__ double a[72][HOM_MODEL_WG];
    __shared__ EpiXY pts[4][HOM_MODEL_WG];
    __shared__ unsigned int sidx[4][HOM_MODEL_WG];
    const int j = blockIdx.y, l = threadIdx.x;
    const unsigned int h = blockIdx.x * HOM_MODEL_WG + l;
    if (h >= NH) return;  // (no barrier below: every lane works on its own columns of the arrays)
    vslam_homography_hyp* out = hyp + (size_t)j * NH + h;
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = false;
    const unsigned int m = g3_count(counts, j, mcap);
    do {
        if (m < 4) break;
        // the sample
        const unsigned int base = epi_mix(epi_mix(seed + (unsigned int)j) + h);
        int n = 0;
        for (unsigned int t = 0; t < 64 && n < 4; ++t) {
            const unsigned int r = epi_mix(base + t);
            const unsigned int i = (unsigned int)(((unsigned long long)r * m) >> 32);
            bool seen = false;
            for (int k = 0; k < n; ++k) seen |= sidx[k][l] == i;
            if (!seen) sidx[n++][l] = i;
        }
        if (n < 4) break;
        bool trusted = true;
        for (int i = 0; i < 4; ++i) {
            const EpiXY p = xy[(size_t)j * mcap + sidx[i][l]];
            trusted &= p.x == p.x && p.u == p.u;
            pts[i][l] = p;
        }
        if (!trusted) break;
        // 1. normalise each side
        double cqx, cqy, sq, ctx, cty, st;
        if (!hom_normalise([&](int i) { return pts[i][l].x; }, [&](int i) { return pts[i][l].y; }, cqx, cqy, sq)) break;
        if (!hom_normalise([&](int i) { return pts[i][l].u; }, [&](int i) { return pts[i][l].v; }, ctx, cty, st)) break;
        // 2. the 8 x 9 matrix
        for (int i = 0; i < 4; ++i) {
            const EpiXY p = pts[i][l];
            const double x = (p.x - cqx) * sq, y = (p.y - cqy) * sq, u = (p.u - ctx) * st, v = (p.v - cty) * st;
            const int r0 = 18 * i, r1 = 18 * i + 9;
            a[r0 + 0][l] = x, a[r0 + 1][l] = y, a[r0 + 2][l] = 1.0;
            a[r0 + 3][l] = 0.0, a[r0 + 4][l] = 0.0, a[r0 + 5][l] = 0.0;
            a[r0 + 6][l] = -(u * x), a[r0 + 7][l] = -(u * y), a[r0 + 8][l] = -u;
            a[r1 + 0][l] = 0.0, a[r1 + 1][l] = 0.0, a[r1 + 2][l] = 0.0;
            a[r1 + 3][l] = x, a[r1 + 4][l] = y, a[r1 + 5][l] = 1.0;
            a[r1 + 6][l] = -(v * x), a[r1 + 7][l] = -(v * y), a[r1 + 8][l] = -v;
        }
        // 3. Gauss-Jordan, full pivoting
        unsigned int used = 0, pcs = 0;  // chosen columns: bit mask, and 4 bits per step
        bool solved = true;
        for (int k = 0; k < 8; ++k) {
            double best = 0.0;
            int pr = -1, pc = -1;
            for (int r = k; r < 8; ++r)
                for (int c = 0; c < 9; ++c) {
                    if (used >> c & 1u) continue;
                    const double v = fabs(a[9 * r + c][l]);
                    if (v > best) best = v, pr = r, pc = c;
                }
            if (pr < 0 || !(best < __longlong_as_double(0x7ff0000000000000ll))) {
                solved = false;
                break;
            }
            if (pr != k)
                for (int c = 0; c < 9; ++c) {
                    const double t = a[9 * k + c][l];
                    a[9 * k + c][l] = a[9 * pr + c][l];
                    a[9 * pr + c][l] = t;
                }
            const double p = a[9 * k + pc][l];
            double rowk[9];
#pragma unroll
            for (int c = 0; c < 9; ++c) {
                rowk[c] = a[9 * k + c][l] / p;
                a[9 * k + c][l] = rowk[c];
            }
            for (int r = 0; r < 8; ++r) {
                if (r == k) continue;
                const double g = a[9 * r + pc][l];
#pragma unroll
                for (int c = 0; c < 9; ++c) a[9 * r + c][l] = a[9 * r + c][l] - g * rowk[c];
            }
            used |= 1u << pc;
            pcs |= (unsigned int)pc << (4 * k);
        }
        if (!solved) break;
        const int fr = __ffs((int)(~used & 0x1ffu)) - 1;
        // h lives in row 0's slots from here on (the matrix is no longer needed once the free column is read out)
        double fk[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) fk[k] = -a[9 * k + fr][l];
        a[fr][l] = 1.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) a[(pcs >> (4 * k)) & 15u][l] = fk[k];
        double hn[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) hn[i] = a[i][l];
        // 4. - 7. the normalisation undone, Frobenius norm 1, the sign (the sample's first record maps to the front), and the
        // way back G = adj(H) under the same sign rule: kernels_geom3.hip.h's, shared with the refit of H
        double Hc[9], Gc[9];
        const EpiXY p0 = pts[0][l];
        if (!hom_denormalise(hn, cqx, cqy, sq, ctx, cty, st, Hc)) break;
        if (!hom_sign(Hc, p0.x, p0.y)) break;
        if (!hom_adjugate(Hc, p0.u, p0.v, Gc)) break;
#pragma unroll
        for (int i = 0; i < 9; ++i) H[i] = Hc[i], G[i] = Gc[i];
        ok = true;
    } while (false);
#pragma unroll
    for (int i = 0; i < 9; ++i) out->H[i] = H[i], out->G[i] = G[i];
    out->inliers = 0;
    out->valid = ok ? 1 : 0;
}

// grid = (hypothesis blocks of 256, nsplit, pairs).  Lane = hypothesis; the workgroup's record tiles (tile index = blockIdx.y
// + k * nsplit) are staged in LDS and every lane walks them in step: the LDS address is the same in all lanes.  The lane's
// integer count goes into its hypothesis by atomicAdd: integer sums merge exactly in any order.
__global__ __launch_bounds__(EPI_SCORE_WG) void k_hom_score(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts,
                                                             unsigned int mcap, unsigned int NH, double max_dist2,
                                                             vslam_homography_hyp* __restrict__ hyp) {
    __shared__ EpiXY tile[EPI_TILE];
    const int j = blockIdx.z;
    const unsigned int m = g3_count(counts, j, mcap);
    const unsigned int h = blockIdx.x * EPI_SCORE_WG + threadIdx.x;
    vslam_homography_hyp* mine = hyp + (size_t)j * NH + min(h, NH - 1);
    double H[9], G[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = mine->H[i], G[i] = mine->G[i];
    const EpiXY* src = xy + (size_t)j * mcap;
    unsigned int count = 0;
    for (size_t t0 = (size_t)blockIdx.y * EPI_TILE; t0 < m; t0 += (size_t)gridDim.y * EPI_TILE) {  // block-uniform trip count
        const unsigned int n = (unsigned int)min((size_t)EPI_TILE, m - t0);
        __syncthreads();
        static_assert(EPI_TILE == EPI_SCORE_WG, "one record per lane when a tile is staged");
        if (threadIdx.x < n) tile[threadIdx.x] = src[t0 + threadIdx.x];
        __syncthreads();
        if (n == EPI_TILE) {
#pragma unroll 4
            for (unsigned int i = 0; i < EPI_TILE; ++i) count += hom_inlier(H, G, tile[i], max_dist2) ? 1u : 0u;
        } else {
            for (unsigned int i = 0; i < n; ++i) count += hom_inlier(H, G, tile[i], max_dist2) ? 1u : 0u;
        }
    }
    if (h < NH && count) atomicAdd(&mine->inliers, count);
}

// grid = (pairs).  The verdict's two fields are written as "no verdict"; k_hom_verdict overwrites them when the call has
// epipolar models.
__global__ __launch_bounds__(256) void k_hom_select(const vslam_homography_hyp* __restrict__ hyp, const unsigned int* __restrict__ counts,
                                                     unsigned int mcap, unsigned int NH, vslam_homography* __restrict__ models) {
    const int j = blockIdx.x;
    ransac_select<HomModel>(hyp + (size_t)j * NH, NH, models + j, [&](vslam_homography& out) {
        out.n_matches = g3_count(counts, j, mcap);
        out.n_epipolar = 0;
        out.degenerate = 0;
    });
}

// grid = (record blocks, pairs)
__global__ __launch_bounds__(256) void k_hom_flags(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                    const vslam_homography* __restrict__ models, double max_dist2,
                                                    unsigned long long* __restrict__ flags, unsigned int fwords) {
    ransac_flags<HomModel>(xy, counts, mcap, models, max_dist2, flags, fwords);
}

// grid = (pair blocks of 64).  One lane per pair, integers only.  `gated` may be the very buffer `epi` points to (neither is
// __restrict__): a lane reads its own record before it writes it and touches no other.
__global__ __launch_bounds__(HOM_PAIR_WG) void k_hom_verdict(const vslam_epipolar* epi, int n_pairs, unsigned int num, unsigned int den,
                                                              unsigned int min_inliers, vslam_homography* __restrict__ models,
                                                              vslam_epipolar* gated) {
    const int j = blockIdx.x * HOM_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    vslam_epipolar e = epi[j];
    const unsigned int nh = models[j].n_inliers, ne = e.best >= 0 ? e.n_inliers : 0u;
    const bool deg = models[j].best >= 0 && e.best >= 0 && nh >= min_inliers &&
                     (unsigned long long)nh * den >= (unsigned long long)num * ne;
    models[j].n_epipolar = ne;
    models[j].degenerate = deg ? 1 : 0;
    if (gated) {
        if (deg) {
#pragma unroll
            for (int i = 0; i < 9; ++i) e.F[i] = 0.0;
            e.n_inliers = 0;
            e.best = -1;
        }
        gated[j] = e;
    }
}

}  // namespace vslam
