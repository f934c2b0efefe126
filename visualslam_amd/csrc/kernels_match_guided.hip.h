// Guided matching (include/vslam.h, "guided matching"): the nearest-two search of kernels_match.hip.h restricted, per query row,
// to the train rows in the query's epipolar band under the pair's fundamental matrix.  d2 is the matcher's (the same MFMA chain,
// the same two norm vectors); the band is one f64 predicate per (query, train) element in the epilogue, grouped exactly as the
// header writes it so that every operation rounds on its own (the unit is compiled with -ffp-contract=off).
//   k_guided_rows        : one thread per row.  A query row gets {a0, a1, a2, a0*a0 + a1*a1} with a = F x; a train row gets
//                          {x', y', b0*b0, b1*b1} with b = F^T x'.  NaN in every field: the row is not trusted, or (query side)
//                          the pair has best < 0 - every comparison with it is then false, which is "not in band".
//                          Per element that leaves  e = (x'*a0 + y'*a1) + a2;  e*e < max_dist2 * ((na + bb0) + bb1).
//   k_match_guided       : k_match_nn2's tiling and MFMA chain.  What a lane knows about its 16 query rows beyond the running
//                          (best, second, index) lives in LDS, not in registers (the f64 coefficients alone would be 128 VGPRs):
//                          s_qa, one GuidedRow per query row of the tile, and s_qn {norm, octave}; the 32 lanes of a half read
//                          the same row, a broadcast.  The train tile's GuidedRows are staged with the tile (s_tc).  An element
//                          that is not in band gets d2 = +inf before the selection, which is the header's "skipped".
//   k_match_guided_merge : k_match_merge with the max_desc_dist2 clause in the acceptance.
// The kernels of kernels_match.hip.h are not touched: these are siblings; match_merge, MatchPart, the tile constants and the guided
// searches' row helpers (guided_xy, GuidedQn) are shared (kernels_match_common.hip.h), and the norms come from the matcher's k_desc_norms (enqueue_desc_norms, vslam_launch.h).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_match_common.hip.h"
#include "vslam_guided_plan.h"

namespace vslam {

// grid = (ceil(cap / GUIDED_ROW_WG), pairs); rows [pair][S.cap]
template <bool QUERY>
__global__ __launch_bounds__(GUIDED_ROW_WG) void k_guided_rows(const vslam_desc_sets S, const vslam_epipolar* __restrict__ models,
                                                               GuidedRow* __restrict__ rows) {
    const int p = blockIdx.y;
    const unsigned int r = blockIdx.x * GUIDED_ROW_WG + threadIdx.x;
    if (r >= min(S.counts[p], S.cap)) return;
    const double nan = guided_nan();
    GuidedRow out{{nan, nan, nan, nan}};
    double x, y;
    if (guided_xy(S.points[(size_t)p * S.cap + r], x, y) && (!QUERY || models[p].best >= 0)) {
        const double* F = models[p].F;
        if (QUERY) {
            const double a0 = (F[0] * x + F[1] * y) + F[2], a1 = (F[3] * x + F[4] * y) + F[5], a2 = (F[6] * x + F[7] * y) + F[8];
            out = GuidedRow{{a0, a1, a2, a0 * a0 + a1 * a1}};
        } else {
            const double b0 = (F[0] * x + F[3] * y) + F[6], b1 = (F[1] * x + F[4] * y) + F[7];
            out = GuidedRow{{x, y, b0 * b0, b1 * b1}};
        }
    }
    rows[(size_t)p * S.cap + r] = out;
}

// Query rows whose LDS reads the epilogue of k_match_guided keeps in flight together.  From the compiler's resource report:
// 1 -> 252 / 248 VGPRs (same_octave on / off), no scratch; 2 -> 256 with 4 spilled / 248; 4 -> 256 with 24 spilled / 256.
constexpr int GUIDED_ROWS_IN_FLIGHT = 1;

// grid = (ceil(Q.cap / MT_Q), nsplit, pairs).  part: [pair][split][Q.cap].  The MFMA chain, the LDS image of a train tile and the
// C / D map are k_match_nn2's (kernels_match.hip.h).
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
    // the query tile's rows: thread t < MT_Q stages row t (a row past the count repeats the last one, as operand A does; it is never written out)
    if (t < MT_Q) {
        const size_t qrow = (size_t)p * Q.cap + min(qbase + t, nq - 1);
        s_qa[t] = qrows[qrow];
        s_qn[t] = GuidedQn{qnorm[qrow], SAME_OCT ? Q.points[qrow].octave : 0};
    }
    float best[16], second[16];
    int index[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        best[r] = second[r] = inf;
        index[r] = -1;
    }

    // one train tile: 64 rows x 16 groups of eight floats, four groups per thread; norm and octave of row t by thread t < 64; one f64
    // of the tile's 64 GuidedRows by every thread
    const unsigned int ntiles = (nt + MT_T - 1) / MT_T;
    float4 pf[8];
    float pnb = 0.0f;
    int ptk = 0;
    double ptc = 0.0;
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
        {
            const unsigned int j = tile * MT_T + (t >> 2);
            ptc = j < nt ? trows[(size_t)p * T.cap + j].v[t & 3] : guided_nan();
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
        s_tc[t] = ptc;
    };

    const float4* b0p = s_b + (col * MT_LD) / 4 + h;
    const float4* b1p = s_b + ((32 + col) * MT_LD) / 4 + h;
    unsigned int tile = split;
    if (tile < ntiles) gload(tile);
    while (tile < ntiles) {
        __syncthreads();  // the previous tile has been read (and, the first time, nothing yet: s_qa / s_qn are published by the next barrier)
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
            const int tc = 32 * blk + col;
            const float nb = s_nb[tc];
            const int tk = s_tk[tc];
            const double xp = s_tc[4 * tc + 0], yp = s_tc[4 * tc + 1], bb0 = s_tc[4 * tc + 2], bb1 = s_tc[4 * tc + 3];
            const int j = (int)(tile * MT_T) + tc;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qr = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const GuidedRow qa = s_qa[qr];
                const GuidedQn qn = s_qn[qr];
                const double e = (xp * qa.v[0] + yp * qa.v[1]) + qa.v[2];
                const bool in_band = e * e < max_dist2 * ((qa.v[3] + bb0) + bb1);
                const float s = acc[r];
                float d2 = (qn.norm + nb) - 2.0f * s;
                if (SAME_OCT && qn.octave != tk) d2 = inf;
                if (!in_band) d2 = inf;
                const bool lt = d2 < best[r];
                const float s2 = d2 < second[r] ? d2 : second[r];
                second[r] = lt ? best[r] : s2;
                index[r] = lt ? j : index[r];
                best[r] = lt ? d2 : best[r];
                // the scheduler may not pull the next rows' LDS reads up past this point: with all 16 rows' coefficients in flight
                // at once (160 registers) the kernel spills; GUIDED_ROWS_IN_FLIGHT rows' worth hides the read latency
                if (r % GUIDED_ROWS_IN_FLIGHT == GUIDED_ROWS_IN_FLIGHT - 1) __builtin_amdgcn_sched_barrier(0);
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
__global__ __launch_bounds__(256) void k_match_guided_merge(const vslam_desc_sets Q, const MatchPart* __restrict__ part, int nsplit, float ratio2,
                                                             float max_desc_dist2, vslam_nn2* __restrict__ nn,
                                                             unsigned long long* __restrict__ flags, unsigned int fwords) {
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
        accept = i >= 0 && (s == inf || b < __fmul_rn(ratio2, s)) && b < max_desc_dist2;
    }
    const unsigned long long w = __ballot(accept);
    if ((threadIdx.x & 63) == 0 && q / 64 < fwords) flags[(size_t)p * fwords + q / 64] = w;
}

}  // namespace vslam
