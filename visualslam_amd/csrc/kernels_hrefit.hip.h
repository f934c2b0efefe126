// Least-squares refit of the homography (include/vslam.h, "homography: least-squares refit over the inliers").  The launch
// structure is kernels_refit.hip.h's, a round = count -> begin -> dist -> scale -> moments -> solve, and so is everything the
// two stages have in common (kernels_geom3.hip.h: refit_block_sums, refit_pair_sums, refit_tree, refit_scales, the 9 x 9
// Jacobi; hom_inlier, hom_denormalise, hom_sign, hom_adjugate).  The streaming kernels, grid = (blocks of 4096 records, pairs),
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
#include "kernels_geom3.hip.h"
#include "vslam_hrefit_plan.h"

namespace vslam {

// true: this workgroup has nothing to do - its pair has stopped, or its block lies past the pair's count.
__device__ __forceinline__ bool hrefit_idle(const HRefitState* __restrict__ state, const unsigned int* __restrict__ counts, unsigned int mcap) {
    return state[blockIdx.y].stop != REFIT_RUNNING || (size_t)blockIdx.x * REFIT_BLOCK >= g3_count(counts, blockIdx.y, mcap);
}

__global__ __launch_bounds__(REFIT_WG) void k_hrefit_count(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                            const HRefitState* __restrict__ state, double max_dist2, double* __restrict__ partial,
                                                            unsigned int sum_blocks) {
    __shared__ double lds[5 * 128];
    if (hrefit_idle(state, counts, mcap)) return;
    double H[9], G[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = state[blockIdx.y].Hcand[k], G[k] = state[blockIdx.y].Gcand[k];
    const auto member = [&](const EpiXY& p) { return hom_inlier(H, G, p, max_dist2); };
    refit_block_sums<5, (int)HREFIT_SUMS>(xy, counts, mcap, partial, sum_blocks, lds, member, [](double (&s)[5], const EpiXY& p) {
        s[0] = s[0] + p.x, s[1] = s[1] + p.y, s[2] = s[2] + p.u, s[3] = s[3] + p.v, s[4] = s[4] + 1.0;
    });
}

__global__ __launch_bounds__(REFIT_WG) void k_hrefit_dist(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                           const HRefitState* __restrict__ state, double max_dist2, double* __restrict__ partial,
                                                           unsigned int sum_blocks) {
    __shared__ double lds[2 * 128];
    if (hrefit_idle(state, counts, mcap)) return;
    const HRefitState* st = state + blockIdx.y;
    double H[9], G[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = st->Hcur[k], G[k] = st->Gcur[k];
    const double cqx = st->cqx, cqy = st->cqy, ctx = st->ctx, cty = st->cty;
    const auto member = [&](const EpiXY& p) { return hom_inlier(H, G, p, max_dist2); };
    refit_block_sums<2, (int)HREFIT_SUMS>(xy, counts, mcap, partial, sum_blocks, lds, member, [=](double (&s)[2], const EpiXY& p) {
        const double dx = p.x - cqx, dy = p.y - cqy, du = p.u - ctx, dv = p.v - cty;
        s[0] = s[0] + sqrt(dx * dx + dy * dy);
        s[1] = s[1] + sqrt(du * du + dv * dv);
    });
}

// The sums lie as [A_0 .. A_5, B_0 .. B_5, C_0 .. C_5, D_0 .. D_5], k = the index pairs (0,0), (0,1), (0,2), (1,1), (1,2), (2,2).
__global__ __launch_bounds__(REFIT_WG) void k_hrefit_moments(const EpiXY* __restrict__ xy, const unsigned int* __restrict__ counts, unsigned int mcap,
                                                              const HRefitState* __restrict__ state, double max_dist2, double* __restrict__ partial,
                                                              unsigned int sum_blocks) {
    __shared__ double lds[HREFIT_SUMS * 128];  // 24576 bytes
    if (hrefit_idle(state, counts, mcap)) return;
    const HRefitState* st = state + blockIdx.y;
    double H[9], G[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) H[k] = st->Hcur[k], G[k] = st->Gcur[k];
    const double cqx = st->cqx, cqy = st->cqy, ctx = st->ctx, cty = st->cty, sq = st->sq, stt = st->st;
    const auto member = [&](const EpiXY& p) { return hom_inlier(H, G, p, max_dist2); };
    refit_block_sums<(int)HREFIT_SUMS, (int)HREFIT_SUMS>(xy, counts, mcap, partial, sum_blocks, lds, member, [=](double (&s)[HREFIT_SUMS], const EpiXY& p) {
        const double x = (p.x - cqx) * sq, y = (p.y - cqy) * sq, u = (p.u - ctx) * stt, v = (p.v - cty) * stt;
        const double w = u * u + v * v;
        const double e[6] = {x * x, x * y, x, y * y, y, 1.0};
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            s[k] = s[k] + e[k];
            s[6 + k] = s[6 + k] + u * e[k];
            s[12 + k] = s[12 + k] + v * e[k];
            s[18 + k] = s[18 + k] + w * e[k];
        }
    });
}

// grid = (pair blocks of 64), one lane per pair - as are the three kernels after it.
__global__ __launch_bounds__(REFIT_PAIR_WG) void k_hrefit_init(const vslam_homography* __restrict__ models_in, int n_pairs, HRefitState* __restrict__ state) {
    const int j = blockIdx.x * REFIT_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    HRefitState s;
    s.in = models_in[j];
#pragma unroll
    for (int k = 0; k < 9; ++k) s.Hcur[k] = s.Hcand[k] = s.in.H[k], s.Gcur[k] = s.Gcand[k] = s.in.G[k];
    s.cqx = s.cqy = s.ctx = s.cty = s.sq = s.st = 0.0;
    s.n_cur = s.n_before = s.accepted = 0;
    s.stop = s.in.best < 0 ? 5 : REFIT_RUNNING;
    state[j] = s;
}

// `models` may be the buffer k_hrefit_init read: it is written by the last launch only (r == rounds), so neither is __restrict__.
__global__ __launch_bounds__(REFIT_PAIR_WG) void k_hrefit_begin(const double* __restrict__ partial, unsigned int sum_blocks,
                                                                 const unsigned int* __restrict__ counts, unsigned int mcap, int n_pairs,
                                                                 unsigned int r, unsigned int rounds, HRefitState* __restrict__ state,
                                                                 vslam_homography* models, vslam_hrefit* __restrict__ info) {
    const int j = blockIdx.x * REFIT_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    HRefitState* st = state + j;
    if (st->stop == REFIT_RUNNING) {
        double s[5];
        refit_pair_sums<5, (int)HREFIT_SUMS>(partial, j, sum_blocks, g3_count(counts, j, mcap), s);
        const unsigned int n = (unsigned int)s[4];
        bool running = true;
        if (r == 0) {
            st->n_before = st->n_cur = n;
        } else if (n >= st->n_cur) {  // step 6
#pragma unroll
            for (int k = 0; k < 9; ++k) st->Hcur[k] = st->Hcand[k], st->Gcur[k] = st->Gcand[k];
            st->n_cur = n;
            st->accepted += 1;
        } else {
            st->stop = 4;
            running = false;
        }
        if (running) {
            if (r == rounds) {
                st->stop = 0;
            } else if (st->n_cur < 4) {  // step 1
                st->stop = 1;
            } else {  // step 2, the centroids
                const double nd = (double)st->n_cur;
                st->cqx = s[0] / nd, st->cqy = s[1] / nd, st->ctx = s[2] / nd, st->cty = s[3] / nd;
            }
        }
    }
    if (r == rounds) {
        vslam_homography out = st->in;
        if (st->stop != 5) {
#pragma unroll
            for (int k = 0; k < 9; ++k) out.H[k] = st->Hcur[k], out.G[k] = st->Gcur[k];
            out.n_inliers = st->n_cur;
        }
        models[j] = out;
        if (info) info[j] = vslam_hrefit{st->n_before, st->n_cur, st->accepted, st->stop};
    }
}

__global__ __launch_bounds__(REFIT_PAIR_WG) void k_hrefit_scale(const double* __restrict__ partial, unsigned int sum_blocks,
                                                                 const unsigned int* __restrict__ counts, unsigned int mcap, int n_pairs,
                                                                 HRefitState* __restrict__ state) {
    const int j = blockIdx.x * REFIT_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    HRefitState* st = state + j;
    if (st->stop != REFIT_RUNNING) return;
    double s[2];
    refit_pair_sums<2, (int)HREFIT_SUMS>(partial, j, sum_blocks, g3_count(counts, j, mcap), s);
    if (!refit_scales(s, st->n_cur, st->sq, st->st)) st->stop = 2;
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
    for (int i = 0; i < 9; ++i) st->Hcand[i] = Hn[i], st->Gcand[i] = Gn[i];
}

}  // namespace vslam
