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
#include "kernels_geom3.hip.h"
#include "vslam_refit_plan.h"

namespace vslam {

// (refit_tree<N>, the tree of the ordered sum over the 256 slots, is kernels_geom3.hip.h's: the resection's refinement sums the same way.
// So are refit_block_sums, refit_pair_sums, refit_scales and the 9 x 9 Jacobi: the refit of the homography, kernels_hrefit.hip.h,
// runs the same text under its own membership predicate.)

// true: this workgroup has nothing to do - its pair has stopped, or its block lies past the pair's count.
__device__ __forceinline__ bool refit_idle(const RefitState* __restrict__ state, const unsigned int* __restrict__ counts, unsigned int mcap) {
    return state[blockIdx.y].stop != REFIT_RUNNING || (size_t)blockIdx.x * REFIT_BLOCK >= g3_count(counts, blockIdx.y, mcap);
}

__global__ __launch_bounds__(REFIT_WG) void k_refit_count(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                           const RefitState* __restrict__ state, double max_dist2, double* __restrict__ partial,
                                                           unsigned int sum_blocks) {
    __shared__ double lds[5 * 128];
    if (refit_idle(state, counts, mcap)) return;
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = state[blockIdx.y].Fcand[k];
    const auto member = [&](const EpiXY& p) { return epi_inlier(F, p, max_dist2); };
    refit_block_sums<5, (int)REFIT_SUMS>(xy, counts, mcap, partial, sum_blocks, lds, member, [](double (&s)[5], const EpiXY& p) {
        s[0] = s[0] + p.x, s[1] = s[1] + p.y, s[2] = s[2] + p.u, s[3] = s[3] + p.v, s[4] = s[4] + 1.0;
    });
}

__global__ __launch_bounds__(REFIT_WG) void k_refit_dist(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                          const RefitState* __restrict__ state, double max_dist2, double* __restrict__ partial,
                                                          unsigned int sum_blocks) {
    __shared__ double lds[2 * 128];
    if (refit_idle(state, counts, mcap)) return;
    const RefitState* st = state + blockIdx.y;
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = st->Fcur[k];
    const double cqx = st->cqx, cqy = st->cqy, ctx = st->ctx, cty = st->cty;
    const auto member = [&](const EpiXY& p) { return epi_inlier(F, p, max_dist2); };
    refit_block_sums<2, (int)REFIT_SUMS>(xy, counts, mcap, partial, sum_blocks, lds, member, [=](double (&s)[2], const EpiXY& p) {
        const double dx = p.x - cqx, dy = p.y - cqy, du = p.u - ctx, dv = p.v - cty;
        s[0] = s[0] + sqrt(dx * dx + dy * dy);
        s[1] = s[1] + sqrt(du * du + dv * dv);
    });
}

__global__ __launch_bounds__(REFIT_WG) void k_refit_moments(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                             const RefitState* __restrict__ state, double max_dist2, double* __restrict__ partial,
                                                             unsigned int sum_blocks) {
    __shared__ double lds[REFIT_SUMS * 128];  // 46080 bytes
    if (refit_idle(state, counts, mcap)) return;
    const RefitState* st = state + blockIdx.y;
    double F[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) F[k] = st->Fcur[k];
    const double cqx = st->cqx, cqy = st->cqy, ctx = st->ctx, cty = st->cty, sq = st->sq, stt = st->st;
    const auto member = [&](const EpiXY& p) { return epi_inlier(F, p, max_dist2); };
    refit_block_sums<(int)REFIT_SUMS, (int)REFIT_SUMS>(xy, counts, mcap, partial, sum_blocks, lds, member, [=](double (&s)[REFIT_SUMS], const EpiXY& p) {
        const double x = (p.x - cqx) * sq, y = (p.y - cqy) * sq, u = (p.u - ctx) * stt, v = (p.v - cty) * stt;
        const double a[9] = {u * x, u * y, u, v * x, v * y, v, x, y, 1.0};
        int k = 0;
#pragma unroll
        for (int p_ = 0; p_ < 9; ++p_) {
#pragma unroll
            for (int q_ = p_; q_ < 9; ++q_, ++k) s[k] = s[k] + a[p_] * a[q_];
        }
    });
}

// grid = (pair blocks of 64), one lane per pair - as are the three kernels after it.
__global__ __launch_bounds__(REFIT_PAIR_WG) void k_refit_init(const vslam_epipolar* __restrict__ models_in, int n_pairs, RefitState* __restrict__ state) {
    const int j = blockIdx.x * REFIT_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    RefitState s;
    s.in = models_in[j];
#pragma unroll
    for (int k = 0; k < 9; ++k) s.Fcur[k] = s.Fcand[k] = s.in.F[k];
    s.cqx = s.cqy = s.ctx = s.cty = s.sq = s.st = 0.0;
    s.n_cur = s.n_before = s.accepted = 0;
    s.stop = s.in.best < 0 ? 5 : REFIT_RUNNING;
    state[j] = s;
}

// `models` may be the buffer k_refit_init read: it is written by the last launch only (r == rounds), so neither is __restrict__.
__global__ __launch_bounds__(REFIT_PAIR_WG) void k_refit_begin(const double* __restrict__ partial, unsigned int sum_blocks,
                                                                const unsigned int* __restrict__ counts, unsigned int mcap, int n_pairs,
                                                                unsigned int r, unsigned int rounds, RefitState* __restrict__ state,
                                                                vslam_epipolar* models, vslam_refit* __restrict__ info) {
    const int j = blockIdx.x * REFIT_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    RefitState* st = state + j;
    if (st->stop == REFIT_RUNNING) {
        double s[5];
        refit_pair_sums<5, (int)REFIT_SUMS>(partial, j, sum_blocks, g3_count(counts, j, mcap), s);
        const unsigned int n = (unsigned int)s[4];
        bool running = true;
        if (r == 0) {
            st->n_before = st->n_cur = n;
        } else if (n >= st->n_cur) {  // step 6
#pragma unroll
            for (int k = 0; k < 9; ++k) st->Fcur[k] = st->Fcand[k];
            st->n_cur = n;
            st->accepted += 1;
        } else {
            st->stop = 4;
            running = false;
        }
        if (running) {
            if (r == rounds) {
                st->stop = 0;
            } else if (st->n_cur < 8) {  // step 1
                st->stop = 1;
            } else {  // step 2, the centroids
                const double nd = (double)st->n_cur;
                st->cqx = s[0] / nd, st->cqy = s[1] / nd, st->ctx = s[2] / nd, st->cty = s[3] / nd;
            }
        }
    }
    if (r == rounds) {
        vslam_epipolar out = st->in;
        if (st->stop != 5) {
#pragma unroll
            for (int k = 0; k < 9; ++k) out.F[k] = st->Fcur[k];
            out.n_inliers = st->n_cur;
        }
        models[j] = out;
        if (info) info[j] = vslam_refit{st->n_before, st->n_cur, st->accepted, st->stop};
    }
}

__global__ __launch_bounds__(REFIT_PAIR_WG) void k_refit_scale(const double* __restrict__ partial, unsigned int sum_blocks,
                                                                const unsigned int* __restrict__ counts, unsigned int mcap, int n_pairs,
                                                                RefitState* __restrict__ state) {
    const int j = blockIdx.x * REFIT_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    RefitState* st = state + j;
    if (st->stop != REFIT_RUNNING) return;
    double s[2];
    refit_pair_sums<2, (int)REFIT_SUMS>(partial, j, sum_blocks, g3_count(counts, j, mcap), s);
    if (!refit_scales(s, st->n_cur, st->sq, st->st)) st->stop = 2;
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
    for (int i = 0; i < 9; ++i) st->Fcand[i] = Hm[i] / nrm;
}

}  // namespace vslam
