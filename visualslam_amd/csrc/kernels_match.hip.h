// Descriptor matching (include/vslam.h, "descriptor matching"): exact nearest / second-nearest search of every query row
// among the train rows of its pair, squared Euclidean distance as d2(a, b) = (n(a) + n(b)) - 2 s(a, b), where s is the
// k-ascending fmaf chain from +0 and n(a) = s(a, a).  v_mfma_f32_32x32x2_f32 IS that chain (one rounding per product, no
// wider accumulator), so the n_q x 128 by 128 x n_t product runs on the matrix cores and is still a pure function of the
// two rows: tile position, split count and launch shape never change a bit of it.
//   k_desc_norms  : n(row) of every row in use, one thread per row (__fmaf_rn, k ascending)
//   k_match_nn2   : a workgroup owns MT_Q query rows of one pair (operand A, held in registers for the whole kernel) and
//                   walks its share of the train tiles in ascending order (operand B, staged in LDS); the epilogue forms
//                   d2 from the two norm vectors, masks skipped rows and updates a per-lane (best, index, second) per
//                   query row; lanes that share a query row merge lexicographically on (d2, index) at the end
//   k_match_merge : merges the partial results of the workgroups that shared a query tile (train tiles are dealt out
//                   round robin to `nsplit` workgroups so that one small pair still fills the chip), applies the ratio
//                   test, writes vslam_nn2 and one ballot word of accepted queries per 64 rows - the flag words the
//                   count -> scan -> scatter kernels of kernels_compact.hip.h (MatchEntries) turn into the ordered match list
// "second" is the second smallest distance of the multiset (two equal minima give second == best), which is what the
// sequential rule of the header yields; min over (d2, index) and that second are order-independent, so the merges are exact.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_match_common.hip.h"  // MT_Q, MT_T, MT_LD, MT_MAX_SPLIT, MatchPart, match_merge

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
// MFMA number n (0 .. 63) of a tile consumes k = 2 n (lanes 0 .. 31) and then k = 2 n + 1 (lanes 32 .. 63), so the chain runs
// k = 0 .. 127 in order.  A lane of half h therefore needs k = h, 2 + h, 4 + h ...: the LDS rows hold every group of eight
// k as [0 2 4 6 1 3 5 7], which makes those four consecutive MFMA operands one ds_read_b128.
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

    // operand A: row (wave, col) of the query tile, the k of this lane's half
    float a[64];
    {
        const unsigned int qrow = qbase + wave * 32 + col;
        const float4* src = reinterpret_cast<const float4*>(Q.desc + ((size_t)p * Q.cap + min(qrow, nq - 1)) * 128);
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const float4 v0 = src[2 * m], v1 = src[2 * m + 1];
            a[4 * m + 0] = h ? v0.y : v0.x;
            a[4 * m + 1] = h ? v0.w : v0.z;
            a[4 * m + 2] = h ? v1.y : v1.x;
            a[4 * m + 3] = h ? v1.w : v1.z;
        }
    }
    // the 16 query rows of this lane's accumulator registers (the C / D map of the 32 x 32 forms)
    float qn[16], best[16], second[16];
    int qk[16], index[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned int qrow = min(qbase + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h, nq - 1);
        qn[r] = qnorm[(size_t)p * Q.cap + qrow];
        qk[r] = SAME_OCT ? Q.points[(size_t)p * Q.cap + qrow].octave : 0;
        best[r] = second[r] = inf;
        index[r] = -1;
    }

    // one train tile: 64 rows x 16 groups of eight floats, four groups per thread; norm and octave of row t by thread t < 64
    const unsigned int ntiles = (nt + MT_T - 1) / MT_T;
    float4 pf[8];
    float pnb = 0.0f;
    int ptk = 0;
    auto gload = [&](unsigned int tile) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int g = t + 256 * it;
            const unsigned int j = tile * MT_T + (g >> 4);
            if (j < nt) {
                const float4* src = reinterpret_cast<const float4*>(T.desc + ((size_t)p * T.cap + j) * 128 + 8 * (g & 15));
                pf[2 * it] = src[0];
                pf[2 * it + 1] = src[1];
            } else {
                pf[2 * it] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                pf[2 * it + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            }
        }
        if (t < MT_T) {
            const unsigned int j = tile * MT_T + t;
            const bool alive = j < nt && (!T.defined || T.defined[(size_t)p * T.cap + j]);
            pnb = alive ? tnorm[(size_t)p * T.cap + j] : __int_as_float(0x7fc00000);  // NaN: a skipped row never wins
            ptk = SAME_OCT && j < nt ? T.points[(size_t)p * T.cap + j].octave : 0;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int g = t + 256 * it;
            float4* dst = s_b + ((g >> 4) * MT_LD + 8 * (g & 15)) / 4;
            const float4 v0 = pf[2 * it], v1 = pf[2 * it + 1];
            dst[0] = make_float4(v0.x, v0.z, v1.x, v1.z);
            dst[1] = make_float4(v0.y, v0.w, v1.y, v1.w);
        }
        if (t < MT_T) s_nb[t] = pnb, s_tk[t] = ptk;
    };

    const float4* b0p = s_b + (col * MT_LD) / 4 + h;
    const float4* b1p = s_b + ((32 + col) * MT_LD) / 4 + h;
    unsigned int tile = split;
    if (tile < ntiles) gload(tile);
    while (tile < ntiles) {
        __syncthreads();  // the previous tile has been read
        lstore();
        __syncthreads();
        const unsigned int next = tile + nsplit;
        if (next < ntiles) gload(next);  // in flight under the MFMAs
        f32x16 acc0 = 0.0f, acc1 = 0.0f;
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            const float4 b0 = b0p[2 * m], b1 = b1p[2 * m];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 0], b0.x, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 0], b1.x, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 1], b0.y, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 1], b1.y, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 2], b0.z, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 2], b1.z, acc1, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 3], b0.w, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * m + 3], b1.w, acc1, 0, 0, 0);
        }
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
                const bool lt = d2 < best[r];
                const float s2 = d2 < second[r] ? d2 : second[r];
                second[r] = lt ? best[r] : s2;
                index[r] = lt ? j : index[r];
                best[r] = lt ? d2 : best[r];
            }
        };
        select(acc0, 0);
        select(acc1, 1);
        tile = next;
    }

    // the 32 lanes of a half hold 32 disjoint sets of train rows for the same 16 query rows
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float ob = __shfl_xor(best[r], off), os = __shfl_xor(second[r], off);
            const int oi = __shfl_xor(index[r], off);
            match_merge(best[r], second[r], index[r], ob, os, oi);
        }
    }
    if (col == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) s_res[wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h] = MatchPart{best[r], second[r], index[r]};
    }
    __syncthreads();
    if (t < MT_Q && qbase + t < nq) part[((size_t)p * nsplit + split) * Q.cap + qbase + t] = s_res[t];
}

// grid = (ceil(Q.cap / 256), pairs); flags: [pair][fwords], fwords = ceil(Q.cap / 64)
__global__ __launch_bounds__(256) void k_match_merge(const vslam_desc_sets Q, const MatchPart* __restrict__ part, int nsplit, float ratio2,
                                                      vslam_nn2* __restrict__ nn, unsigned long long* __restrict__ flags,
                                                      unsigned int fwords) {
    const int p = blockIdx.y;
    const unsigned int q = blockIdx.x * 256 + threadIdx.x;
    const unsigned int nq = min(Q.counts[p], Q.cap);
    const float inf = match_inf();
    bool accept = false;
    if (q < nq) {
        float b = inf, s = inf;
        int i = -1;
        if (!Q.defined || Q.defined[(size_t)p * Q.cap + q]) {
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
    const unsigned long long w = __ballot(accept);
    if ((threadIdx.x & 63) == 0 && q / 64 < fwords) flags[(size_t)p * fwords + q / 64] = w;
}

}  // namespace vslam
