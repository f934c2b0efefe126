// Guided matching (include/vslam.h, "guided matching"): the nearest-two search of kernels_match.hip.h restricted, per query row,
// to the train rows in the query's epipolar band under the pair's fundamental matrix.  d2 is the matcher's (the same MFMA chain,
// the same two norm vectors); the band is one f64 predicate per (query, train) element in the epilogue, grouped exactly as the
// header writes it so that every operation rounds on its own (the unit is compiled with -ffp-contract=off).
//   k_guided_rows        : one thread per row writes its GuidedRow (guided_row_f); NaN in every field: the row is not trusted, or
//                          (query side) the pair has best < 0 - every comparison with it is then false, which is "not in band".
//   k_match_guided       : guided_search<SAME_OCT, false> for pair blockIdx.z
//   k_match_guided_merge : match_merge_rows with the max_desc_dist2 clause in the acceptance.
// The search itself, the row record and the fold are kernels_match_common.hip.h's, shared with the pass under H or F
// (kernels_match_guided_hf.hip.h); the norms come from the matcher's k_desc_norms (enqueue_desc_norms, vslam_launch.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_match_common.hip.h"

namespace vslam {

// grid = (ceil(cap / MT_ROW_WG), pairs); rows [pair][S.cap]
template <bool QUERY>
__global__ __launch_bounds__(MT_ROW_WG) void k_guided_rows(const vslam_desc_sets S, const vslam_epipolar* __restrict__ models,
                                                           GuidedRow* __restrict__ rows) {
    const int p = blockIdx.y;
    const unsigned int r = blockIdx.x * MT_ROW_WG + threadIdx.x;
    if (r >= min(S.counts[p], S.cap)) return;
    const double nan = guided_nan();
    GuidedRow out{{nan, nan, nan, nan}};
    double x, y;
    if (guided_xy(S.points[(size_t)p * S.cap + r], x, y) && (!QUERY || models[p].best >= 0)) out = guided_row_f<QUERY>(models[p].F, x, y);
    rows[(size_t)p * S.cap + r] = out;
}

// grid = (ceil(Q.cap / MT_Q), nsplit, pairs).  part: [pair][split][Q.cap].
template <bool SAME_OCT>
__global__ __launch_bounds__(256, 2) void k_match_guided(const vslam_desc_sets Q, const vslam_desc_sets T, const float* __restrict__ qnorm,
                                                         const float* __restrict__ tnorm, const GuidedRow* __restrict__ qrows,
                                                         const GuidedRow* __restrict__ trows, double max_dist2, int nsplit,
                                                         MatchPart* __restrict__ part) {
    __shared__ float4 s_b[MT_T * MT_LD / 4];
    __shared__ float s_nb[MT_T];
    __shared__ int s_tk[MT_T];
    __shared__ MatchPart s_res[MT_Q];
    __shared__ GuidedRow s_qa[MT_Q];
    __shared__ GuidedQn s_qn[MT_Q];
    __shared__ __attribute__((aligned(16))) double s_tc[MT_T * 4];  // the tile's GuidedRows, flat
    const int p = blockIdx.z;
    const unsigned int nq = min(Q.counts[p], Q.cap), nt = min(T.counts[p], T.cap);
    if (blockIdx.x * MT_Q >= nq) return;
    guided_search<SAME_OCT, false>(Q, T, qnorm, tnorm, qrows, trows, max_dist2, nsplit, part, p, nq, nt, s_b, s_nb, s_tk, s_res, s_qa, s_qn, s_tc);
}

// grid = (ceil(Q.cap / MT_ROW_WG), pairs)
__global__ __launch_bounds__(256) void k_match_guided_merge(const vslam_desc_sets Q, const MatchPart* __restrict__ part, int nsplit, float ratio2,
                                                             float max_desc_dist2, vslam_nn2* __restrict__ nn,
                                                             unsigned long long* __restrict__ flags, unsigned int fwords) {
    match_merge_rows(Q, part, nsplit, ratio2, nn, flags, fwords, [=](int, unsigned int, float b, int) { return b < max_desc_dist2; });
}

}  // namespace vslam
