// Least-squares refit of the fundamental matrix (include/vslam.h, "fundamental matrix: least-squares refit over the inliers").
// The streaming kernels, grid = (blocks of 4096 records, pairs), 256 lanes = the 256 slots of the header's ordered sum, 16
// coalesced 32-byte records per lane, membership recomputed in every pass (epi_inlier under the pair's F, a broadcast read):
//   k_refit_count   : SUM(x), SUM(y), SUM(x'), SUM(y') and SUM(1.0) - the member count, exact in f64 - under the CANDIDATE F
//   k_refit_dist    : SUM(sqrt(dx*dx + dy*dy)) per side under the kept F
//   k_refit_moments : the 45 sums M[p][q], p <= q, under the kept F
// Each block's sums go to the scratch with plain stores; the per-pair kernels, one lane per pair, add them left to right:
//   k_refit_init    : models_in -> RefitState
//   k_refit_begin   : round r's first steps: the count pass before it belongs to round r - 1's F_new (r >= 1: step 6, accept
//                     or stop 4) or to the input F (r == 0: n_before); then step 1 and the centroids of step 2.  The launch
//                     with r == rounds closes the last round and writes models and info.
//   k_refit_scale   : the rest of step 2
//   k_refit_solve   : steps 3 - 5: the 9 x 9 Jacobi with S and V statically indexed (every loop over p, q, r unrolled), F_new
// No floating-point atomics, no flags or fences between workgroups: kernel boundaries order everything.  A workgroup of a
// stopped pair, or of a block past the pair's count, leaves before its first barrier (workgroup-uniform).  The arithmetic is
// the header's, operation for operation, under the rules of kernels_epipolar.hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_estimate.hip.h"
#include "kernels_geom3.hip.h"
#include "vslam_refit_plan.h"

namespace vslam {

// (What the rounds of this stage and of the homography's share is stated once: kernels_estimate.hip.h has the streaming pass,
// the count and distance sums and the per-pair steps init, begin and scale; kernels_geom3.hip.h the ordered sum - refit_tree,
// refit_block_sums, refit_pair_sums -, refit_scales and the 9 x 9 Jacobi.  This stage's own: the add step of the moments pass
// and steps 3 - 5.)

__global__ __launch_bounds__(REFIT_WG) void k_refit_count(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                           const RefitState* __restrict__ state, double max_dist2, double* __restrict__ partial,
                                                           unsigned int sum_blocks) {
    refit_pass<5, true, RefitCountAdd>(xy, counts, mcap, state, max_dist2, partial, sum_blocks);
}

__global__ __launch_bounds__(REFIT_WG) void k_refit_dist(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                          const RefitState* __restrict__ state, double max_dist2, double* __restrict__ partial,
                                                          unsigned int sum_blocks) {
    refit_pass<2, false, RefitDistAdd>(xy, counts, mcap, state, max_dist2, partial, sum_blocks);
}

// One member's 45 products a[p] * a[q], p <= q, of its row a of step 3; the tree takes 45 x 128 x 8 = 46080 bytes of LDS.
struct RefitMomentsAdd {
    RefitNorm nm;
    __device__ void operator()(double (&s)[REFIT_SUMS], const EpiXY& p) const {
        const double x = (p.x - nm.cqx) * nm.sq, y = (p.y - nm.cqy) * nm.sq, u = (p.u - nm.ctx) * nm.st, v = (p.v - nm.cty) * nm.st;
        const double a[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
        int k = 0;
#pragma unroll
        for (int p_ = 0; p_ < 9; ++p_) {
#pragma unroll
            for (int q_ = p_; q_ < 9; ++q_, ++k) s[k] = s[k] + a[p_] * a[q_];
        }
    }
};
__global__ __launch_bounds__(REFIT_WG) void k_refit_moments(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                             const RefitState* __restrict__ state, double max_dist2, double* __restrict__ partial,
                                                             unsigned int sum_blocks) {
    refit_pass<(int)REFIT_SUMS, false, RefitMomentsAdd>(xy, counts, mcap, state, max_dist2, partial, sum_blocks);
}

// grid = (pair blocks of 64), one lane per pair - as are the three kernels after it.
__global__ __launch_bounds__(REFIT_PAIR_WG) void k_refit_init(const vslam_epipolar* __restrict__ models_in, int n_pairs, RefitState* __restrict__ state) {
    refit_init(models_in, n_pairs, state);
}

// `models` may be the buffer k_refit_init read: it is written by the last launch only (r == rounds), so neither is __restrict__.
__global__ __launch_bounds__(REFIT_PAIR_WG) void k_refit_begin(const double* __restrict__ partial, unsigned int sum_blocks,
                                                                const unsigned int* __restrict__ counts, unsigned int mcap, int n_pairs,
                                                                unsigned int r, unsigned int rounds, RefitState* __restrict__ state,
                                                                vslam_epipolar* models, vslam_refit* __restrict__ info) {
    refit_begin(partial, sum_blocks, counts, mcap, n_pairs, r, rounds, state, models, info);
}

__global__ __launch_bounds__(REFIT_PAIR_WG) void k_refit_scale(const double* __restrict__ partial, unsigned int sum_blocks,
                                                                const unsigned int* __restrict__ counts, unsigned int mcap, int n_pairs,
                                                                RefitState* __restrict__ state) {
    refit_scale(partial, sum_blocks, counts, mcap, n_pairs, state);
}

__global__ __launch_bounds__(REFIT_PAIR_WG) void k_refit_solve(const double* __restrict__ partial, unsigned int sum_blocks,
                                                                const unsigned int* __restrict__ counts, unsigned int mcap, int n_pairs,
                                                                RefitState* __restrict__ state) {
    const int j = blockIdx.x * REFIT_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    RefitState* st = state + j;
    if (st->stop != REFIT_RUNNING) return;
    // 3. the moment matrix: the pair's 45 sums are the upper triangle, row-major
    double S[9][9], V[9][9];
    {
        double s[REFIT_SUMS];
        refit_pair_sums<(int)REFIT_SUMS, (int)REFIT_SUMS>(partial, j, sum_blocks, g3_count(counts, j, mcap), s);
        int k = 0;
#pragma unroll
        for (int p = 0; p < 9; ++p) {
#pragma unroll
            for (int q = 0; q < 9; ++q) V[p][q] = p == q ? 1.0 : 0.0;
#pragma unroll
            for (int q = p; q < 9; ++q, ++k) S[p][q] = s[k];
        }
    }
    // 4. the eigenvector of the smallest eigenvalue
    double f[9];
    refit_smallest_eigenvector(S, V, VSLAM_REFIT_SWEEPS, f);
    // 5. F_new: rank 2, the normalisation undone, Frobenius norm 1
    g3_rank2(f);
    const double sq = st->sq, stt = st->st;
    double Hm[9];
    g3_lt_f_r(G3Affine{stt, stt, -(stt * st->ctx), -(stt * st->cty)}, f, G3Affine{sq, sq, -(sq * st->cqx), -(sq * st->cqy)}, Hm);
    const double nrm = g3_frobenius(Hm);
    if (!g3_finite_nonzero(nrm)) {
        st->stop = 3;
        return;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) st->cand.F[i] = Hm[i] / nrm;
}

}  // namespace vslam
