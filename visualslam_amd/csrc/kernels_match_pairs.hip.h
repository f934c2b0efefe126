// The indexed matcher (include/vslam.h, "loop verification", Match): k_match_nn2's search with the two sets of a pair taken from a
// table on the device.  The arithmetic is the matcher's, step for step (kernels_match_common.hip.h); what differs is addressing:
//   the SET index (pairs[p].query_set / .train_set) goes to match_load_a, match_tile_gload and the norm, count and octave reads;
//   the PAIR index p goes to part, nn and flags.
//   k_match_nn2_pairs   : grid = (ceil(Q.cap / MT_Q), nsplit, n_pairs); a workgroup of an empty pair returns before it reads anything else
//   k_match_merge_pairs : grid = (ceil(Q.cap / MT_ROW_WG), n_pairs); match_merge_rows with the set and the output index apart: the
//                         row count and the `defined` bytes are the query SET's, part / nn / flags the PAIR's.  An empty pair gets
//                         zero flag words (so its match count is 0) and its nn rows stay untouched.
// The norms are those of the sets: qnorm [n_query_sets][Q.cap], tnorm [n_train_sets][T.cap] (k_desc_norms over the sets).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_match_common.hip.h"
#include "vslam_loop_plan.h"  // pair_empty

namespace vslam {

// part: [pair][split][Q.cap]
template <bool SAME_OCT>
__global__ __launch_bounds__(256) void k_match_nn2_pairs(const vslam_desc_sets Q, const vslam_desc_sets T, const vslam_set_pair* __restrict__ pairs,
                                                          unsigned int n_query_sets, unsigned int n_train_sets, const float* __restrict__ qnorm,
                                                          const float* __restrict__ tnorm, int nsplit, MatchPart* __restrict__ part) {
    __shared__ float4 s_b[MT_T * MT_LD / 4];
    __shared__ float s_nb[MT_T];
    __shared__ int s_tk[MT_T];
    __shared__ MatchPart s_res[MT_Q];
    const int p = blockIdx.z, split = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31, h = lane >> 5;
    const vslam_set_pair pr = pairs[p];
    if (pair_empty(pr, n_query_sets, n_train_sets)) return;
    const int qs = pr.query_set, ts = pr.train_set;
    const unsigned int nq = min(Q.counts[qs], Q.cap), nt = min(T.counts[ts], T.cap);
    const unsigned int qbase = blockIdx.x * MT_Q;
    if (qbase >= nq) return;
    const float inf = match_inf();

    float a[64];
    match_load_a(a, Q, qs, min(qbase + wave * 32 + col, nq - 1), h);
    // the 16 query rows of this lane's accumulator registers
    float qn[16], best[16], second[16];
    int qk[16], index[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned int qrow = min(qbase + wave * 32 + match_cd_row(r, h), nq - 1);
        qn[r] = qnorm[(size_t)qs * Q.cap + qrow];
        qk[r] = SAME_OCT ? Q.points[(size_t)qs * Q.cap + qrow].octave : 0;
        best[r] = second[r] = inf;
        index[r] = -1;
    }

    const unsigned int ntiles = (nt + MT_T - 1) / MT_T;
    float4 pf[8];
    float pnb = 0.0f;
    int ptk = 0;
    const float4 *b0p = match_b_ptr(s_b, 0, col, h), *b1p = match_b_ptr(s_b, 1, col, h);
    unsigned int tile = split;
    if (tile < ntiles) match_tile_gload<SAME_OCT>(pf, pnb, ptk, T, tnorm, ts, nt, tile, t);
    while (tile < ntiles) {
        __syncthreads();  // the previous tile has been read
        match_tile_lstore(pf, pnb, ptk, s_b, s_nb, s_tk, t);
        __syncthreads();
        const unsigned int next = tile + nsplit;
        if (next < ntiles) match_tile_gload<SAME_OCT>(pf, pnb, ptk, T, tnorm, ts, nt, next, t);  // in flight under the MFMAs
        f32x16 acc0, acc1;
        match_mfma_chain(a, b0p, b1p, acc0, acc1);
        // epilogue: this lane's train column of each block against its 16 query rows, ascending train index
        auto select = [&](const f32x16& acc, int blk) {
            const float nb = s_nb[32 * blk + col];
            const int tk = s_tk[32 * blk + col];
            const int j = (int)(tile * MT_T) + 32 * blk + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s = acc[r];
                float d2 = (qn[r] + nb) - 2.0f * s;
                if (SAME_OCT && qk[r] != tk) d2 = inf;
                match_nn2_update(best, second, index, r, d2, j);
            }
        };
        select(acc0, 0);
        select(acc1, 1);
        tile = next;
    }
    match_finish(best, second, index, s_res, part, Q, p, nsplit, split, qbase, nq, t, wave, col, h);  // part is the PAIR's
}

__global__ __launch_bounds__(256) void k_match_merge_pairs(const vslam_desc_sets Q, const vslam_set_pair* __restrict__ pairs, unsigned int n_query_sets,
                                                            unsigned int n_train_sets, const MatchPart* __restrict__ part, int nsplit, float ratio2,
                                                            vslam_nn2* __restrict__ nn, unsigned long long* __restrict__ flags, unsigned int fwords) {
    const int p = blockIdx.y;
    const unsigned int q = blockIdx.x * MT_ROW_WG + threadIdx.x;
    const vslam_set_pair pr = pairs[p];
    const bool empty = pair_empty(pr, n_query_sets, n_train_sets);  // (the same in every lane of the workgroup)
    const float inf = match_inf();
    bool accept = false;
    if (!empty) {
        const int qs = pr.query_set;
        const unsigned int nq = min(Q.counts[qs], Q.cap);
        if (q < nq) {
            float b = inf, s = inf;
            int i = -1;
            if (!Q.defined || Q.defined[(size_t)qs * Q.cap + q]) {
                for (int k = 0; k < nsplit; ++k) {
                    const MatchPart o = part[((size_t)p * nsplit + k) * Q.cap + q];
                    match_merge(b, s, i, o.best, o.second, o.index);
                }
            }
            vslam_nn2 r;
            r.index = i;
            r.dist2 = b;
            r.second_dist2 = s;
            nn[(size_t)p * Q.cap + q] = r;
            accept = i >= 0 && (s == inf || b < __fmul_rn(ratio2, s));
        }
    }
    const unsigned long long w = __ballot(accept);
    if ((threadIdx.x & 63) == 0 && q / 64 < fwords) flags[(size_t)p * fwords + q / 64] = w;
}

}  // namespace vslam
