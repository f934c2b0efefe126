// Two-view geometry (include/vslam.h, "two-view geometry"): RANSAC fundamental matrix of every pair of a batch.
//   k_epi_coords : one lane per match record -> {x, y, x', y'} f64 in image pixels (NaN: the record is not trusted)
//   k_epi_models : one lane per (pair, hypothesis): sample 8 records, normalised 8-point model, rank 2 by Jacobi
//   k_epi_score  : the hot path, pairs x hypotheses x records Sampson tests: one lane per hypothesis with F in registers,
//                  the workgroup walks record tiles staged in LDS (every lane reads the same address: a broadcast)
//   k_epi_select : one workgroup per pair: the valid hypothesis with the most inliers, lowest index on ties
//   k_epi_flags  : the winner's inlier ballot words; kernels_compact.hip.h (EpipolarEntries) turns them into the list
// The last two are the shared RANSAC steps of kernels_estimate.hip.h under this stage's model; k_epi_score keeps its own text
// (behind an inlined body its scalar prologue is scheduled otherwise: profiles/estimators_isa_identity.txt).
// The arithmetic is the header's, operation for operation: every + - * / sqrt of f64 is an IEEE operation of its own (the
// library is built with -ffp-contract=off; f64 division and sqrt are correctly rounded on gfx950), sums run left to right.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_estimate.hip.h"
#include "kernels_geom3.hip.h"
#include "vslam_epipolar_plan.h"

namespace vslam {

// grid = (record blocks, pairs)
__global__ __launch_bounds__(256) void k_epi_coords(const vslam_match* __restrict__ matches, const unsigned int* __restrict__ counts,
                                                     unsigned int mcap, const vslam_point* __restrict__ qpts, unsigned int qcap,
                                                     const vslam_point* __restrict__ tpts, unsigned int tcap, EpiXY* __restrict__ xy) {
    const int j = blockIdx.y;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // (64 bits: the last block of a capacity near 2^32 runs past it)
    if (i >= g3_count(counts, j, mcap)) return;
    const vslam_match m = matches[(size_t)j * mcap + i];
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    EpiXY r{nan, nan, nan, nan};
    if ((unsigned int)m.query < qcap && (unsigned int)m.train < tcap) {
        const vslam_point q = qpts[(size_t)j * qcap + (unsigned int)m.query], t = tpts[(size_t)j * tcap + (unsigned int)m.train];
        if ((unsigned int)q.octave <= 31u && (unsigned int)t.octave <= 31u) {
            const double sq = q.octave == 0 ? 0.5 : (double)(1u << (q.octave - 1));
            const double st = t.octave == 0 ? 0.5 : (double)(1u << (t.octave - 1));
            r.x = (double)((long long)q.col - (long long)q.padding) * sq;
            r.y = (double)((long long)q.row - (long long)q.padding) * sq;
            r.u = (double)((long long)t.col - (long long)t.padding) * st;
            r.v = (double)((long long)t.row - (long long)t.padding) * st;
        }
    }
    xy[(size_t)j * mcap + i] = r;
}

// Step 1 of the model for one side: the 8 values are read through `get(i)`.
template <class GetX, class GetY>
__device__ __forceinline__ bool epi_normalise(GetX gx, GetY gy, double& cx, double& cy, double& s) {
    double sx = gx(0), sy = gy(0);
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        sx = sx + gx(i);
        sy = sy + gy(i);
    }
    cx = sx / 8.0;
    cy = sy / 8.0;
    double d = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double dx = gx(i) - cx, dy = gy(i) - cy;
        const double r = sqrt(dx * dx + dy * dy);
        d = i == 0 ? r : d + r;
    }
    d = d / 8.0;
    if (d == 0.0) return false;
    s = 1.4142135623730951 / d;
    return true;
}

// grid = (hypothesis blocks of 64, pairs), one wave.  The 8 x 9 matrix is indexed by a data-dependent pivot, so it lives in
// LDS, lane-strided: element e of lane l at a[e][l] - the 64 lanes of one access hit 64 consecutive f64, no bank conflict.
__global__ __launch_bounds__(EPI_MODEL_WG) void k_epi_models(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts,
                                                              unsigned int mcap, unsigned int H, unsigned int seed,
                                                              vslam_epipolar_hyp* __restrict__ hyp) {
    __shared__ double a[72][EPI_MODEL_WG];
    __shared__ EpiXY pts[8][EPI_MODEL_WG];
    __shared__ unsigned int sidx[8][EPI_MODEL_WG];
    const int j = blockIdx.y, l = threadIdx.x;
    const unsigned int h = blockIdx.x * EPI_MODEL_WG + l;
    if (h >= H) return;  // (no barrier below: every lane works on its own columns of the arrays)
    vslam_epipolar_hyp* out = hyp + (size_t)j * H + h;
    double F[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    bool ok = false;
    const unsigned int m = g3_count(counts, j, mcap);
    do {
        if (m < 8) break;
        // the sample
        const unsigned int base = epi_mix(epi_mix(seed + (unsigned int)j) + h);
        int n = 0;
        for (unsigned int t = 0; t < 64 && n < 8; ++t) {
            const unsigned int r = epi_mix(base + t);
            const unsigned int i = (unsigned int)(((unsigned long long)r * m) >> 32);
            bool seen = false;
            for (int k = 0; k < n; ++k) seen |= sidx[k][l] == i;
            if (!seen) sidx[n++][l] = i;
        }
        if (n < 8) break;
        bool trusted = true;
        for (int i = 0; i < 8; ++i) {
            const EpiXY p = xy[(size_t)j * mcap + sidx[i][l]];
            trusted &= p.x == p.x && p.u == p.u;
            pts[i][l] = p;
        }
        if (!trusted) break;
        // 1. normalise each side
        double cqx, cqy, sq, ctx, cty, st;
        if (!epi_normalise([&](int i) { return pts[i][l].x; }, [&](int i) { return pts[i][l].y; }, cqx, cqy, sq)) break;
        if (!epi_normalise([&](int i) { return pts[i][l].u; }, [&](int i) { return pts[i][l].v; }, ctx, cty, st)) break;
        // 2. the 8 x 9 matrix
        for (int i = 0; i < 8; ++i) {
            const EpiXY p = pts[i][l];
            const double x = (p.x - cqx) * sq, y = (p.y - cqy) * sq, u = (p.u - ctx) * st, v = (p.v - cty) * st;
            a[9 * i + 0][l] = u * x;
            a[9 * i + 1][l] = u * y;
            a[9 * i + 2][l] = u;
            a[9 * i + 3][l] = v * x;
            a[9 * i + 4][l] = v * y;
            a[9 * i + 5][l] = v;
            a[9 * i + 6][l] = x;
            a[9 * i + 7][l] = y;
            a[9 * i + 8][l] = 1.0;
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
        // f lives in row 0's slots from here on (the matrix is no longer needed once the free column is read out)
        double fk[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) fk[k] = -a[9 * k + fr][l];
        a[fr][l] = 1.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) a[(pcs >> (4 * k)) & 15u][l] = fk[k];
        double f[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) f[i] = a[i][l];
        // 4. rank 2: the singular vector of the smallest singular value is projected out
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
        // 5. undo the normalisation
        double Hm[9];
        g3_lt_f_r(G3Affine{st, st, -(st * ctx), -(st * cty)}, f, G3Affine{sq, sq, -(sq * cqx), -(sq * cqy)}, Hm);
        // 6. Frobenius norm 1
        const double nrm = g3_frobenius(Hm);
        if (!g3_finite_nonzero(nrm)) break;
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = Hm[i] / nrm;
        ok = true;
    } while (false);
#pragma unroll
    for (int i = 0; i < 9; ++i) out->F[i] = F[i];
    out->inliers = 0;
    out->valid = ok ? 1 : 0;
}

// grid = (hypothesis blocks of 256, nsplit, pairs).  Lane = hypothesis; the workgroup's record tiles (tile index = blockIdx.y
// + k * nsplit) are staged in LDS and every lane walks them in step: the LDS address is the same in all lanes.  The lane's
// integer count goes into its hypothesis by atomicAdd: integer sums merge exactly in any order.
__global__ __launch_bounds__(EPI_SCORE_WG) void k_epi_score(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts,
                                                             unsigned int mcap, unsigned int H, double max_dist2,
                                                             vslam_epipolar_hyp* __restrict__ hyp) {
    __shared__ EpiXY tile[EPI_TILE];
    const int j = blockIdx.z;
    const unsigned int m = g3_count(counts, j, mcap);
    const unsigned int h = blockIdx.x * EPI_SCORE_WG + threadIdx.x;
    vslam_epipolar_hyp* mine = hyp + (size_t)j * H + min(h, H - 1);
    double F[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) F[i] = mine->F[i];
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
            for (unsigned int i = 0; i < EPI_TILE; ++i) count += epi_inlier(F, tile[i], max_dist2) ? 1u : 0u;
        } else {
            for (unsigned int i = 0; i < n; ++i) count += epi_inlier(F, tile[i], max_dist2) ? 1u : 0u;
        }
    }
    if (h < H && count) atomicAdd(&mine->inliers, count);
}

// grid = (pairs)
__global__ __launch_bounds__(256) void k_epi_select(const vslam_epipolar_hyp* __restrict__ hyp, const unsigned int* __restrict__ counts,
                                                     unsigned int mcap, unsigned int H, vslam_epipolar* __restrict__ models) {
    const int j = blockIdx.x;
    ransac_select<EpiModel>(hyp + (size_t)j * H, H, models + j, [&](vslam_epipolar& out) { out.n_matches = g3_count(counts, j, mcap); });
}

// grid = (record blocks, pairs)
__global__ __launch_bounds__(256) void k_epi_flags(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                    const vslam_epipolar* __restrict__ models, double max_dist2,
                                                    unsigned long long* __restrict__ flags, unsigned int fwords) {
    ransac_flags<EpiModel>(xy, counts, mcap, models, max_dist2, flags, fwords);
}

}  // namespace vslam
