// Least-squares refit of the homography (include/vslam.h, "homography: least-squares refit over the inliers").  The launch
// structure is kernels_refit.hip.h's, a round = count -> begin -> dist -> scale -> moments -> solve, and so is everything the
// two stages have in common (kernels_estimate.hip.h: the streaming pass, the count and distance sums, init, begin and scale;
// kernels_geom3.hip.h: refit_block_sums, refit_pair_sums, refit_tree, refit_scales, the 9 x 9 Jacobi; hom_inlier,
// hom_denormalise, hom_sign, hom_adjugate).  This stage's own: the add step of the moments pass and steps 3 - 5.  The streaming kernels, grid = (blocks of 4096 records, pairs),
// 256 lanes = the 256 slots of the header's ordered sum, membership recomputed in every pass (hom_inlier under the pair's
// (H, G), a broadcast read):
//   k_hrefit_count   : SUM(x), SUM(y), SUM(x'), SUM(y') and SUM(1.0) - the member count, exact in f64 - under the CANDIDATE model
//   k_hrefit_dist    : SUM(sqrt(dx*dx + dy*dy)) per side under the kept model
//   k_hrefit_moments : the 24 sums A_k, B_k, C_k, D_k under the kept model - the hot kernel: 24 accumulators per lane, a tree
//                      of 24 x 128 x 8 = 24576 bytes of LDS
// and the per-pair kernels, one lane per pair:
//   k_hrefit_init    : models_in -> HRefitState
//   k_hrefit_begin   : step 6 of the round before (or n_before), step 1 and the centroids of step 2; the launch with
//                      r == rounds closes the last round and writes models and info
//   k_hrefit_scale   : the rest of step 2
//   k_hrefit_solve   : steps 3 - 5: M from the 24 sums through its block structure, the Jacobi, (H_new, G_new)
// The verdict is k_hom_verdict's and the ballot words k_hom_flags' (vslam_homography.hip compiles them).  No floating-point
// atomics, no flags or fences between workgroups: kernel boundaries order everything.  A workgroup of a stopped pair, or of a
// block past the pair's count, leaves before its first barrier (workgroup-uniform).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_estimate.hip.h"
#include "kernels_geom3.hip.h"
#include "vslam_hrefit_plan.h"

namespace vslam {

__global__ __launch_bounds__(REFIT_WG) void k_hrefit_count(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                            const HRefitState* __restrict__ state, double max_dist2, double* __restrict__ partial,
                                                            unsigned int sum_blocks) {
    refit_pass<5, true, RefitCountAdd>(xy, counts, mcap, state, max_dist2, partial, sum_blocks);
}

__global__ __launch_bounds__(REFIT_WG) void k_hrefit_dist(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                           const HRefitState* __restrict__ state, double max_dist2, double* __restrict__ partial,
                                                           unsigned int sum_blocks) {
    refit_pass<2, false, RefitDistAdd>(xy, counts, mcap, state, max_dist2, partial, sum_blocks);
}

// One member's 24 terms.  The sums lie as [A_0 .. A_5, B_0 .. B_5, C_0 .. C_5, D_0 .. D_5], k = the index pairs (0,0), (0,1),
// (0,2), (1,1), (1,2), (2,2).
struct HRefitMomentsAdd {
    RefitNorm nm;
    __device__ void operator()(double (&s)[HREFIT_SUMS], const EpiXY& p) const {
        const double x = (p.x - nm.cqx) * nm.sq, y = (p.y - nm.cqy) * nm.sq, u = (p.u - nm.ctx) * nm.st, v = (p.v - nm.cty) * nm.st;
        const double w = u * u + v * v;
        const double e[6] = {x * x, x * y, x, y * y, y, 1.0};
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            s[k] = s[k] + e[k];
            s[6 + k] = s[6 + k] + u * e[k];
            s[12 + k] = s[12 + k] + v * e[k];
            s[18 + k] = s[18 + k] + w * e[k];
        }
    }
};
__global__ __launch_bounds__(REFIT_WG) void k_hrefit_moments(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                              const HRefitState* __restrict__ state, double max_dist2, double* __restrict__ partial,
                                                              unsigned int sum_blocks) {
    refit_pass<(int)HREFIT_SUMS, false, HRefitMomentsAdd>(xy, counts, mcap, state, max_dist2, partial, sum_blocks);
}

// grid = (pair blocks of 64), one lane per pair - as are the three kernels after it.
__global__ __launch_bounds__(REFIT_PAIR_WG) void k_hrefit_init(const vslam_homography* __restrict__ models_in, int n_pairs, HRefitState* __restrict__ state) {
    refit_init(models_in, n_pairs, state);
}

// `models` may be the buffer k_hrefit_init read: it is written by the last launch only (r == rounds), so neither is __restrict__.
__global__ __launch_bounds__(REFIT_PAIR_WG) void k_hrefit_begin(const double* __restrict__ partial, unsigned int sum_blocks,
                                                                 const unsigned int* __restrict__ counts, unsigned int mcap, int n_pairs,
                                                                 unsigned int r, unsigned int rounds, HRefitState* __restrict__ state,
                                                                 vslam_homography* models, vslam_hrefit* __restrict__ info) {
    refit_begin(partial, sum_blocks, counts, mcap, n_pairs, r, rounds, state, models, info);
}

__global__ __launch_bounds__(REFIT_PAIR_WG) void k_hrefit_scale(const double* __restrict__ partial, unsigned int sum_blocks,
                                                                 const unsigned int* __restrict__ counts, unsigned int mcap, int n_pairs,
                                                                 HRefitState* __restrict__ state) {
    refit_scale(partial, sum_blocks, counts, mcap, n_pairs, state);
}

__global__ __launch_bounds__(REFIT_PAIR_WG) void k_hrefit_solve(const double* __restrict__ partial, unsigned int sum_blocks,
                                                                 const unsigned int* __restrict__ counts, unsigned int mcap, int n_pairs,
                                                                 HRefitState* __restrict__ state) {
    const int j = blockIdx.x * REFIT_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    HRefitState* st = state + j;
    if (st->stop != REFIT_RUNNING) return;
    // 3. the moment matrix, upper triangle, through its block structure: k(a, b) is compile-time in every use
    double S[9][9], V[9][9];
    {
        double s[HREFIT_SUMS];
        refit_pair_sums<(int)HREFIT_SUMS, (int)HREFIT_SUMS>(partial, j, sum_blocks, g3_count(counts, j, mcap), s);
#pragma unroll
        for (int p = 0; p < 9; ++p) {
#pragma unroll
            for (int q = 0; q < 9; ++q) V[p][q] = p == q ? 1.0 : 0.0;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const int lo = a < b ? a : b, hi = a < b ? b : a;
                const int k = lo == 0 ? hi : lo + hi + 1;  // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) -> 0 .. 5
                if (a <= b) S[a][b] = S[3 + a][3 + b] = s[k], S[6 + a][6 + b] = s[18 + k];
                S[a][3 + b] = 0.0;
                S[a][6 + b] = -s[6 + k];
                S[3 + a][6 + b] = -s[12 + k];
            }
        }
    }
    // 4. the eigenvector of the smallest eigenvalue
    double h[9];
    refit_smallest_eigenvector(S, V, VSLAM_HREFIT_SWEEPS, h);
    // 5. (H_new, G_new): the normalisation undone, Frobenius norm 1, the signs from the members' centroids
    double Hn[9], Gn[9];
    if (!hom_denormalise(h, st->cqx, st->cqy, st->sq, st->ctx, st->cty, st->st, Hn) || !hom_sign(Hn, st->cqx, st->cqy) ||
        !hom_adjugate(Hn, st->ctx, st->cty, Gn)) {
        st->stop = 3;
        return;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) st->cand.H[i] = Hn[i], st->cand.G[i] = Gn[i];
}

}  // namespace vslam
