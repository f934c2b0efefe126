// Guided matching under H or F (include/vslam.h, "guided matching under H or F"): the guided pass of kernels_match_guided.hip.h
// with the candidate predicate chosen per pair - the epipolar band where the pair has an F, a window around H x where it has
// only an H, nothing where it has neither.  The kind is read on the device from the two model arrays (guided_kind); blockIdx.z
// (the rows kernel: blockIdx.y) is the pair, so the choice is uniform per workgroup.
//   k_guided_hf_rows  : one thread per row, one 32-byte GuidedRow per row.  Kind F: k_guided_rows' two records (guided_row_f).
//                       Kind H, query row: {p0, p1, p2, L} with p = H x and L = max_transfer2 * (p2*p2), NaN in
//                       every field when the row is not trusted or p2 > 0 is false; train row: {x', y', 0, 0}, NaN when not
//                       trusted.  Kind NONE: NaN.  Per element that leaves, under H,
//                       dx = p0 - x'*p2;  dy = p1 - y'*p2;  dx*dx + dy*dy < L  - seven f64 operations against the band's nine.
//   k_match_guided_hf : k_match_guided's search (guided_search, kernels_match_common.hip.h) with the element predicate a template
//                       parameter and the pair taken from a list.  A call launches the F form when it has epipolar
//                       models and the H form when it has homography models; with both, each form takes its pairs from the
//                       list k_guided_hf_kinds wrote and the workgroups past the list's end leave before they load anything,
//                       so no pair's tiles go through the matrix cores twice.  Two kernels, not one that branches: with both
//                       epilogues in one kernel the compiler spills (256 VGPRs and 32 / 48 bytes of scratch per lane with
//                       same_octave off / on).  A NONE pair runs no MFMA: its workgroups - of the H form when the call has
//                       homography models, else of the F form - write the "nothing found" partial results, which
//                       k_match_guided_merge turns into {-1, +inf, +inf} rows and a count of 0.
//   k_guided_hf_kinds : the pairs of a call sorted by kind, for a call with both model arrays.
// The merge, its acceptance and the list compaction are the guided pass's, as they are (enqueue_guided_merge, vslam_launch.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_match_common.hip.h"
#include "vslam_guided_hf_plan.h"

namespace vslam {

__device__ __forceinline__ int guided_kind(const vslam_epipolar* __restrict__ emodels, const vslam_homography* __restrict__ hmodels, int p) {
    if (emodels && emodels[p].best >= 0) return GUIDED_KIND_F;
    if (hmodels && hmodels[p].best >= 0) return GUIDED_KIND_H;
    return GUIDED_KIND_NONE;
}

// grid = (ceil(cap / MT_ROW_WG), pairs); rows [pair][S.cap]
template <bool QUERY>
__global__ __launch_bounds__(MT_ROW_WG) void k_guided_hf_rows(const vslam_desc_sets S, const vslam_epipolar* __restrict__ emodels,
                                                                  const vslam_homography* __restrict__ hmodels, double max_transfer2,
                                                                  GuidedRow* __restrict__ rows) {
    const int p = blockIdx.y;
    const unsigned int r = blockIdx.x * MT_ROW_WG + threadIdx.x;
    if (r >= min(S.counts[p], S.cap)) return;
    const double nan = guided_nan();
    GuidedRow out{{nan, nan, nan, nan}};
    const int kind = guided_kind(emodels, hmodels, p);
    double x, y;
    if (kind != GUIDED_KIND_NONE && guided_xy(S.points[(size_t)p * S.cap + r], x, y)) {
        if (kind == GUIDED_KIND_F) {
            out = guided_row_f<QUERY>(emodels[p].F, x, y);
        } else if (QUERY) {
            const double* H = hmodels[p].H;
            const double p0 = (H[0] * x + H[1] * y) + H[2], p1 = (H[3] * x + H[4] * y) + H[5], p2 = (H[6] * x + H[7] * y) + H[8];
            if (p2 > 0.0) out = GuidedRow{{p0, p1, p2, max_transfer2 * (p2 * p2)}};
        } else {
            out = GuidedRow{{x, y, 0.0, 0.0}};
        }
    }
    rows[(size_t)p * S.cap + r] = out;
}

// One workgroup: the pairs of a call sorted by kind, ascending within each - list [2][n_pairs] with the F pairs in row 0 and the H
// pairs followed by the NONE pairs (bit 31 set) in row 1, count [2] the entries of each row.  The search takes its pair from the
// list of its form, so that the workgroups with work are the first of the grid whatever the order of the kinds in the call: with
// blockIdx.z the pair itself, kinds that alternate put the working workgroups of each form on every other slot of the
// dispatcher's round, and half the compute units idle (measured: 2.0 x the time at 255 pairs of 2 k rows).  Thread t counts the
// kinds of its stretch of pairs, thread 0 turns the counts into offsets, thread t writes its stretch: no atomic, one order.
__global__ __launch_bounds__(MT_ROW_WG) void k_guided_hf_kinds(const vslam_epipolar* __restrict__ emodels, const vslam_homography* __restrict__ hmodels,
                                                                   int n_pairs, unsigned int* __restrict__ list, unsigned int* __restrict__ count) {
    __shared__ unsigned int s_n[3][MT_ROW_WG];  // per thread: F, H, NONE pairs of its stretch, then their offsets
    const int t = threadIdx.x, per = (n_pairs + MT_ROW_WG - 1) / MT_ROW_WG;
    const int lo = min(t * per, n_pairs), hi = min(lo + per, n_pairs);
    unsigned int n[3] = {0, 0, 0};
    for (int p = lo; p < hi; ++p) {
        const int kind = guided_kind(emodels, hmodels, p);
        n[kind == GUIDED_KIND_F ? 0 : kind == GUIDED_KIND_H ? 1 : 2] += 1;
    }
    for (int k = 0; k < 3; ++k) s_n[k][t] = n[k];
    __syncthreads();
    if (t == 0) {
        const int used = (n_pairs + per - 1) / per;  // threads with a stretch: a one-pair call walks one entry, not 256
        unsigned int at[3] = {0, 0, 0};
        for (int i = 0; i < used; ++i)
            for (int k = 0; k < 3; ++k) {
                const unsigned int c = s_n[k][i];
                s_n[k][i] = at[k];
                at[k] += c;
            }
        for (int i = 0; i < used; ++i) s_n[2][i] += at[1];  // the NONE pairs follow the H pairs
        count[0] = at[0];
        count[1] = at[1] + at[2];
    }
    __syncthreads();
    unsigned int at[3] = {s_n[0][t], s_n[1][t], s_n[2][t]};
    for (int p = lo; p < hi; ++p) {
        const int kind = guided_kind(emodels, hmodels, p);
        if (kind == GUIDED_KIND_F) list[at[0]++] = (unsigned int)p;
        else if (kind == GUIDED_KIND_H) list[(size_t)n_pairs + at[1]++] = (unsigned int)p;
        else list[(size_t)n_pairs + at[2]++] = (unsigned int)p | 0x80000000u;
    }
}

// grid = (ceil(Q.cap / MT_Q), nsplit, pairs).  part: [pair][split][Q.cap].
template <bool SAME_OCT, bool KIND_H>
__global__ __launch_bounds__(256, 2) void k_match_guided_hf(const vslam_desc_sets Q, const vslam_desc_sets T, const float* __restrict__ qnorm,
                                                            const float* __restrict__ tnorm, const GuidedRow* __restrict__ qrows,
                                                            const GuidedRow* __restrict__ trows, const vslam_epipolar* __restrict__ emodels,
                                                            const vslam_homography* __restrict__ hmodels, const unsigned int* __restrict__ list,
                                                            const unsigned int* __restrict__ count, double max_dist2, int nsplit,
                                                            MatchPart* __restrict__ part) {
    __shared__ float4 s_b[MT_T * MT_LD / 4];
    __shared__ float s_nb[MT_T];
    __shared__ int s_tk[MT_T];
    __shared__ MatchPart s_res[MT_Q];
    __shared__ GuidedRow s_qa[MT_Q];
    __shared__ GuidedQn s_qn[MT_Q];
    __shared__ __attribute__((aligned(16))) double s_tc[MT_T * 4];  // the tile's GuidedRows, flat
    const int split = blockIdx.y, t = threadIdx.x;
    // the pair: entry blockIdx.z of this form's list (k_guided_hf_kinds), or blockIdx.z itself in a call with one model array
    if (list && blockIdx.z >= count[KIND_H]) return;
    const unsigned int entry = list ? list[(KIND_H ? (size_t)gridDim.z : 0) + blockIdx.z] : blockIdx.z;
    const int p = (int)(entry & 0x7fffffffu);
    const unsigned int nq = min(Q.counts[p], Q.cap), nt = min(T.counts[p], T.cap);
    const unsigned int qbase = blockIdx.x * MT_Q;
    if (qbase >= nq) return;
    const float inf = match_inf();
    const int kind = list ? (entry >> 31 ? GUIDED_KIND_NONE : KIND_H ? GUIDED_KIND_H : GUIDED_KIND_F) : guided_kind(emodels, hmodels, p);
    if (kind != (KIND_H ? GUIDED_KIND_H : GUIDED_KIND_F)) {
        // a pair without a model (the H form's list holds them; without a list this form is the only one): nothing found, and no MFMA
        if (kind == GUIDED_KIND_NONE && t < MT_Q && qbase + t < nq) part[((size_t)p * nsplit + split) * Q.cap + qbase + t] = MatchPart{inf, inf, -1};
        return;
    }
    guided_search<SAME_OCT, KIND_H>(Q, T, qnorm, tnorm, qrows, trows, max_dist2, nsplit, part, p, nq, nt, s_b, s_nb, s_tk, s_res, s_qa, s_qn, s_tc);
}

}  // namespace vslam
