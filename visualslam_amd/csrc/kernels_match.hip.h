// Descriptor matching (include/vslam.h, "descriptor matching"): exact nearest / second-nearest search of every query row
// among the train rows of its pair, squared Euclidean distance as d2(a, b) = (n(a) + n(b)) - 2 s(a, b), where s is the
// k-ascending fmaf chain from +0 and n(a) = s(a, a).  v_mfma_f32_32x32x2_f32 IS that chain (one rounding per product, no
// wider accumulator), so the n_q x 128 by 128 x n_t product runs on the matrix cores and is still a pure function of the
// two rows: tile position, split count and launch shape never change a bit of it.
//   k_desc_norms  : n(row) of every row in use, one thread per row (__fmaf_rn, k ascending)
//   k_match_nn2   : a workgroup owns MT_Q query rows of one pair (operand A, held in registers for the whole kernel) and
//                   walks its share of the train tiles in ascending order (operand B, staged in LDS); the epilogue forms
//                   d2 from the two norm vectors, masks skipped rows and updates a per-lane (best, index, second) per
//                   query row; lanes that share a query row merge lexicographically on (d2, index) at the end.  The
//                   steps of that walk are the ones every search of the family takes (kernels_match_common.hip.h).
//   k_match_merge : merges the partial results of the workgroups that shared a query tile (train tiles are dealt out
//                   round robin to `nsplit` workgroups so that one small pair still fills the chip), applies the ratio
//                   test, writes vslam_nn2 and one ballot word of accepted queries per 64 rows - the flag words the
//                   count -> scan -> scatter kernels of kernels_compact.hip.h (MatchEntries) turn into the ordered match list
// "second" is the second smallest distance of the multiset (two equal minima give second == best), which is what the
// sequential rule of the header yields; min over (d2, index) and that second are order-independent, so the merges are exact.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_match_common.hip.h"

namespace vslam {

// grid = (ceil(cap / 256), pairs)
__global__ __launch_bounds__(256) void k_desc_norms(const vslam_desc_sets S, float* __restrict__ norms) {
    const int p = blockIdx.y;
    const unsigned int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= min(S.counts[p], S.cap)) return;
    const float4* row = reinterpret_cast<const float4*>(S.desc + ((size_t)p * S.cap + r) * 128);
    float acc = 0.0f;
    for (int k = 0; k < 32; ++k) {
        const float4 v = row[k];
        acc = __fmaf_rn(v.x, v.x, acc);
        acc = __fmaf_rn(v.y, v.y, acc);
        acc = __fmaf_rn(v.z, v.z, acc);
        acc = __fmaf_rn(v.w, v.w, acc);
    }
    norms[(size_t)p * S.cap + r] = acc;
}

// grid = (ceil(Q.cap / MT_Q), nsplit, pairs).  part: [pair][split][Q.cap].
template <bool SAME_OCT>
__global__ __launch_bounds__(256) void k_match_nn2(const vslam_desc_sets Q, const vslam_desc_sets T, const float* __restrict__ qnorm,
                                                    const float* __restrict__ tnorm, int nsplit, MatchPart* __restrict__ part) {
    __shared__ float4 s_b[MT_T * MT_LD / 4];
    __shared__ float s_nb[MT_T];
    __shared__ int s_tk[MT_T];
    __shared__ MatchPart s_res[MT_Q];
    const int p = blockIdx.z, split = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31, h = lane >> 5;
    const unsigned int nq = min(Q.counts[p], Q.cap), nt = min(T.counts[p], T.cap);
    const unsigned int qbase = blockIdx.x * MT_Q;
    if (qbase >= nq) return;
    const float inf = match_inf();

    float a[64];
    match_load_a(a, Q, p, min(qbase + wave * 32 + col, nq - 1), h);
    // the 16 query rows of this lane's accumulator registers
    float qn[16], best[16], second[16];
    int qk[16], index[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned int qrow = min(qbase + wave * 32 + match_cd_row(r, h), nq - 1);
        qn[r] = qnorm[(size_t)p * Q.cap + qrow];
        qk[r] = SAME_OCT ? Q.points[(size_t)p * Q.cap + qrow].octave : 0;
        best[r] = second[r] = inf;
        index[r] = -1;
    }

    const unsigned int ntiles = (nt + MT_T - 1) / MT_T;
    float4 pf[8];
    float pnb = 0.0f;
    int ptk = 0;
    const float4 *b0p = match_b_ptr(s_b, 0, col, h), *b1p = match_b_ptr(s_b, 1, col, h);
    unsigned int tile = split;
    if (tile < ntiles) match_tile_gload<SAME_OCT>(pf, pnb, ptk, T, tnorm, p, nt, tile, t);
    while (tile < ntiles) {
        __syncthreads();  // the previous tile has been read
        match_tile_lstore(pf, pnb, ptk, s_b, s_nb, s_tk, t);
        __syncthreads();
        const unsigned int next = tile + nsplit;
        if (next < ntiles) match_tile_gload<SAME_OCT>(pf, pnb, ptk, T, tnorm, p, nt, next, t);  // in flight under the MFMAs
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
    match_finish(best, second, index, s_res, part, Q, p, nsplit, split, qbase, nq, t, wave, col, h);
}

// grid = (ceil(Q.cap / MT_ROW_WG), pairs): match_merge_rows with nothing added to the acceptance
__global__ __launch_bounds__(256) void k_match_merge(const vslam_desc_sets Q, const MatchPart* __restrict__ part, int nsplit, float ratio2,
                                                      vslam_nn2* __restrict__ nn, unsigned long long* __restrict__ flags,
                                                      unsigned int fwords) {
    match_merge_rows(Q, part, nsplit, ratio2, nn, flags, fwords, [](int, unsigned int, float, int) { return true; });
}

}  // namespace vslam
