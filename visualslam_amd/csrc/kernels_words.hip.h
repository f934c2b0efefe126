// Visual words (include/vslam.h, "place recognition"): the nearest vocabulary row of every descriptor row, and the histogram of
// words per set.  The search is the matcher's (kernels_match.hip.h) with one train side for every set - the K vocabulary rows -
// and the nearest only: the same steps of kernels_match_common.hip.h in the same loop, so d2 is the same pure function of the two
// rows and a word is what vslam_match_dev would write as nn.index against the vocabulary.
//   k_vocab_gather : word k <- one 512-byte row of the sets, by the header's rule (32 lanes x 16 bytes per word)
//   k_words_nn     : a workgroup owns MT_Q rows of one set (operand A, in registers) and walks its share of the vocabulary tiles
//                    in ascending order (operand B, staged in LDS); the epilogue forms d2 from the two norm vectors and keeps a
//                    per-lane (best, index) per row; the lanes that share a row merge on (d2, index) at the end
//   k_words_merge  : folds the nsplit partial results of a row (match_merge, the fold of match_merge_rows, without the second),
//                    writes words / word_dist2 and adds the row to its bin of the histogram: one integer atomic add per row
// The vocabulary's norms come from k_desc_norms over the vocabulary as a one-set vslam_desc_sets.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_match_common.hip.h"
#include "vslam_place_plan.h"

namespace vslam {

struct WordPart {  // what one workgroup knows about one row
    float best;
    int index;
};

// (b, i) <- the nearer of two disjoint sets of words: match_merge, whose second-nearest the compiler drops
__device__ __forceinline__ void words_fold(float& b, int& i, float ob, int oi) {
    float s = match_inf();
    match_merge(b, s, i, ob, match_inf(), oi);
}

// grid = ceil(K / PL_GATHER_WG), 256 lanes: 32 lanes copy one row
__global__ __launch_bounds__(256) void k_vocab_gather(const vslam_desc_sets S, unsigned int n_sets, unsigned int K, float* __restrict__ vocab,
                                                      uint8_t* __restrict__ vocab_defined) {
    const unsigned int k = blockIdx.x * PL_GATHER_WG + (threadIdx.x >> 5), lane = threadIdx.x & 31;
    if (k >= K) return;
    const unsigned int s = k % n_sets, rows = min(S.counts[s], S.cap);
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool def = false;
    if (rows > 0) {
        const unsigned int r = ((k / n_sets) * 2654435761u) % rows;
        const size_t at = (size_t)s * S.cap + r;
        def = !S.defined || S.defined[at];
        if (def) v = reinterpret_cast<const float4*>(S.desc + at * 128)[lane];
    }
    reinterpret_cast<float4*>(vocab + (size_t)k * 128)[lane] = v;
    if (lane == 0) vocab_defined[k] = def ? 1 : 0;
}

// grid = (ceil(Q.cap / MT_Q), nsplit, n_sets).  V: the vocabulary as one set (desc, defined, cap = K; set 0 for every workgroup),
// vnorm [K].  part: [set][split][Q.cap].
__global__ __launch_bounds__(256) void k_words_nn(const vslam_desc_sets Q, const vslam_desc_sets V, const float* __restrict__ qnorm,
                                                  const float* __restrict__ vnorm, int nsplit, WordPart* __restrict__ part) {
    __shared__ float4 s_b[MT_T * MT_LD / 4];
    __shared__ float s_nb[MT_T];
    __shared__ int s_tk[MT_T];
    __shared__ WordPart s_res[MT_Q];
    const int f = blockIdx.z, split = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31, h = lane >> 5;
    const unsigned int nq = min(Q.counts[f], Q.cap), nt = V.cap;
    const unsigned int qbase = blockIdx.x * MT_Q;
    if (qbase >= nq) return;
    const float inf = match_inf();

    float a[64];
    match_load_a(a, Q, f, min(qbase + wave * 32 + col, nq - 1), h);
    // the 16 rows of this lane's accumulator registers
    float qn[16], best[16];
    int index[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned int qrow = min(qbase + wave * 32 + match_cd_row(r, h), nq - 1);
        qn[r] = qnorm[(size_t)f * Q.cap + qrow];
        best[r] = inf;
        index[r] = -1;
    }

    const unsigned int ntiles = (nt + MT_T - 1) / MT_T;
    float4 pf[8];
    float pnb = 0.0f;
    int ptk = 0;
    const float4 *b0p = match_b_ptr(s_b, 0, col, h), *b1p = match_b_ptr(s_b, 1, col, h);
    unsigned int tile = split;
    if (tile < ntiles) match_tile_gload<false>(pf, pnb, ptk, V, vnorm, 0, nt, tile, t);
    while (tile < ntiles) {
        __syncthreads();  // the previous tile has been read
        match_tile_lstore(pf, pnb, ptk, s_b, s_nb, s_tk, t);
        __syncthreads();
        const unsigned int next = tile + nsplit;
        if (next < ntiles) match_tile_gload<false>(pf, pnb, ptk, V, vnorm, 0, nt, next, t);  // in flight under the MFMAs
        f32x16 acc0, acc1;
        match_mfma_chain(a, b0p, b1p, acc0, acc1);
        // epilogue: this lane's word of each block against its 16 rows, ascending word index: a strict < keeps the lowest
        auto select = [&](const f32x16& acc, int blk) {
            const float nb = s_nb[32 * blk + col];
            const int j = (int)(tile * MT_T) + 32 * blk + col;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s = acc[r];
                const float d2 = (qn[r] + nb) - 2.0f * s;
                const bool lt = d2 < best[r];
                index[r] = lt ? j : index[r];
                best[r] = lt ? d2 : best[r];
            }
        };
        select(acc0, 0);
        select(acc1, 1);
        tile = next;
    }
    // the 32 lanes of a half hold 32 disjoint sets of words for the same 16 rows
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float ob = __shfl_xor(best[r], off);
            const int oi = __shfl_xor(index[r], off);
            words_fold(best[r], index[r], ob, oi);
        }
    }
    if (col == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s_res[wave * 32 + match_cd_row(r, h)] = WordPart{best[r], index[r]};
    }
    __syncthreads();
    if (t < MT_Q && qbase + t < nq) part[((size_t)f * nsplit + split) * Q.cap + qbase + t] = s_res[t];
}

// grid = (ceil(Q.cap / MT_ROW_WG), n_sets): one thread per row.  words, word_dist2 [set][Q.cap] and hist [set][K] may each be
// null; hist has been zeroed.
__global__ __launch_bounds__(256) void k_words_merge(const vslam_desc_sets Q, const WordPart* __restrict__ part, int nsplit, unsigned int K,
                                                     int* __restrict__ words, float* __restrict__ word_dist2, unsigned int* __restrict__ hist) {
    const int f = blockIdx.y;
    const unsigned int q = blockIdx.x * MT_ROW_WG + threadIdx.x;
    if (q >= min(Q.counts[f], Q.cap)) return;
    float b = match_inf();
    int i = -1;
    if (!Q.defined || Q.defined[(size_t)f * Q.cap + q]) {
        for (int k = 0; k < nsplit; ++k) {
            const WordPart o = part[((size_t)f * nsplit + k) * Q.cap + q];
            words_fold(b, i, o.best, o.index);
        }
    }
    if (words) words[(size_t)f * Q.cap + q] = i;
    if (word_dist2) word_dist2[(size_t)f * Q.cap + q] = b;
    if (hist && i >= 0) atomicAdd(&hist[(size_t)f * K + (unsigned int)i], 1u);
}

}  // namespace vslam
