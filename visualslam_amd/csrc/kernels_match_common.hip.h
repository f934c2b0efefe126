// What the four searches over descriptor rows are made of (kernels_match.hip.h: the matcher; kernels_match_guided.hip.h and
// kernels_match_guided_hf.hip.h: the guided passes; kernels_match_mutual.hip.h: the mutual matcher).  Each search kernel keeps its
// loop over the train tiles, its barriers and its epilogue predicate; the steps of that loop are stated here, once, and take the
// kernel's own registers by reference:
//   match_load_a      operand A, a query row held in registers for the whole kernel
//   match_tile_gload  a train tile's descriptors, norms and octaves, global -> registers (in flight under the previous tile's MFMAs)
//   match_tile_lstore ... registers -> the LDS image the MFMA operands are read from
//   match_mfma_chain  the 128 MFMAs of one tile
//   match_cd_row      the C / D map: which query row an accumulator register holds
//   match_nn2_update  one distance into a lane's running (best, second, index)
//   match_finish      the merge of the lanes that share a query row, and the write of the workgroup's partial results
// then the fold of those partial results (match_merge_rows: the body of the three merge kernels), and the search of the two
// guided passes (guided_search), which differ in how a workgroup finds its pair and nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "vslam_guided_plan.h"  // GuidedRow; MT_Q, MT_T, MT_MAX_SPLIT, MT_ROW_WG (vslam_match_plan.h)

namespace vslam {

// floats per LDS row.  128 would put every row on the same banks; + 4 spreads the 16 lanes that one ds_read_b128 cycle
// serves over all 64 banks (lane j starts at bank 4 j mod 64, and no two lanes of a group are 16 apart)
constexpr int MT_LD = 132;

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct MatchPart {  // what one workgroup knows about one query row
    float best, second;
    int index;
};

__device__ __forceinline__ float match_inf() { return __int_as_float(0x7f800000); }

// (b, s, i) <- the nearest two of the union of two disjoint sets of train rows
__device__ __forceinline__ void match_merge(float& b, float& s, int& i, float ob, float os, int oi) {
    const bool win = ob < b || (ob == b && (unsigned int)oi < (unsigned int)i);
    const float loser = win ? b : ob;
    float ns = os < s ? os : s;
    ns = loser < ns ? loser : ns;
    b = win ? ob : b;
    i = win ? oi : i;
    s = ns;
}

// MFMA number n (0 .. 63) of a tile consumes k = 2 n (lanes 0 .. 31) and then k = 2 n + 1 (lanes 32 .. 63), so the chain runs
// k = 0 .. 127 in order.  A lane of half h therefore needs k = h, 2 + h, 4 + h ...: operand A holds them in that order, and the
// LDS rows hold every group of eight k as [0 2 4 6 1 3 5 7], which makes four consecutive MFMA operands B one ds_read_b128.

// operand A: row `qrow` of pair p's query set, the k of this lane's half
__device__ __forceinline__ void match_load_a(float (&a)[64], const vslam_desc_sets& Q, int p, unsigned int qrow, int h) {
    const float4* src = reinterpret_cast<const float4*>(Q.desc + ((size_t)p * Q.cap + qrow) * 128);
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        const float4 v0 = src[2 * m], v1 = src[2 * m + 1];
        a[4 * m + 0] = h ? v0.y : v0.x;
        a[4 * m + 1] = h ? v0.w : v0.z;
        a[4 * m + 2] = h ? v1.y : v1.x;
        a[4 * m + 3] = h ? v1.w : v1.z;
    }
}

// one train tile: 64 rows x 16 groups of eight floats, four groups per thread; norm and octave of row t by thread t < 64
template <bool SAME_OCT>
__device__ __forceinline__ void match_tile_gload(float4 (&pf)[8], float& pnb, int& ptk, const vslam_desc_sets& T, const float* __restrict__ tnorm,
                                                 int p, unsigned int nt, unsigned int tile, int t) {
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
        pnb = alive ? tnorm[(size_t)p * T.cap + j] : __int_as_float(0x7fc00000);  // NaN: a skipped row never wins, in either direction
        ptk = SAME_OCT && j < nt ? T.points[(size_t)p * T.cap + j].octave : 0;
    }
}

__device__ __forceinline__ void match_tile_lstore(const float4 (&pf)[8], float pnb, int ptk, float4* s_b, float* s_nb, int* s_tk, int t) {
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int g = t + 256 * it;
        float4* dst = s_b + ((g >> 4) * MT_LD + 8 * (g & 15)) / 4;
        const float4 v0 = pf[2 * it], v1 = pf[2 * it + 1];
        dst[0] = make_float4(v0.x, v0.z, v1.x, v1.z);
        dst[1] = make_float4(v0.y, v0.w, v1.y, v1.w);
    }
    if (t < MT_T) s_nb[t] = pnb, s_tk[t] = ptk;
}

// this lane's operands B in the LDS image: train column `col` of 32-column block `blk`, the k of half h
__device__ __forceinline__ const float4* match_b_ptr(const float4* s_b, int blk, int col, int h) { return s_b + ((32 * blk + col) * MT_LD) / 4 + h; }

// acc0 / acc1 <- the wave's 32 query rows against train columns 0 .. 31 / 32 .. 63 of the tile in LDS
__device__ __forceinline__ void match_mfma_chain(const float (&a)[64], const float4* b0p, const float4* b1p, f32x16& acc0, f32x16& acc1) {
    acc0 = 0.0f, acc1 = 0.0f;
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
}

// The C / D map of the 32 x 32 forms: accumulator register r (0 .. 15) of a lane of half h holds row match_cd_row(r, h) of the
// wave's 32 query rows, ascending in r.
__device__ __forceinline__ int match_cd_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// train row j at distance d2 into the running nearest two of accumulator register r; the rows arrive in ascending j, so a strict <
// keeps the lowest index.  (The arrays and r, not three references to elements: that form costs k_match_nn2_mutual<true> 7 VGPRs
// and a spill.)
__device__ __forceinline__ void match_nn2_update(float (&best)[16], float (&second)[16], int (&index)[16], int r, float d2, int j) {
    const bool lt = d2 < best[r];
    const float s2 = d2 < second[r] ? d2 : second[r];
    second[r] = lt ? best[r] : s2;
    index[r] = lt ? j : index[r];
    best[r] = lt ? d2 : best[r];
}

// The end of a search kernel, reached by the whole workgroup: the 32 lanes of a half hold 32 disjoint sets of train rows for the
// same 16 query rows; their merge goes through s_res to part [pair][split][Q.cap].
__device__ __forceinline__ void match_finish(float (&best)[16], float (&second)[16], int (&index)[16], MatchPart* s_res, MatchPart* __restrict__ part,
                                             const vslam_desc_sets& Q, int p, int nsplit, int split, unsigned int qbase, unsigned int nq, int t, int wave,
                                             int col, int h) {
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
        for (int r = 0; r < 16; ++r) s_res[wave * 32 + match_cd_row(r, h)] = MatchPart{best[r], second[r], index[r]};
    }
    __syncthreads();
    if (t < MT_Q && qbase + t < nq) part[((size_t)p * nsplit + split) * Q.cap + qbase + t] = s_res[t];
}

// The body of the merge kernels, grid = (ceil(Q.cap / MT_ROW_WG), pairs): one thread per query row folds the partial results of
// the nsplit workgroups that shared its tile (none for a row that is not defined), writes the row's vslam_nn2, and the wave
// writes one ballot word of accepted rows - flags [pair][fwords], fwords = ceil(Q.cap / 64), which the count -> scan -> scatter
// kernels of kernels_compact.hip.h (MatchEntries) turn into the ordered match list.  Accepted: a neighbour, the ratio test, and
// what the kernel adds, also (pair, query row, best, index) -> bool.
template <typename Also>
__device__ __forceinline__ void match_merge_rows(const vslam_desc_sets& Q, const MatchPart* __restrict__ part, int nsplit, float ratio2,
                                                 vslam_nn2* __restrict__ nn, unsigned long long* __restrict__ flags, unsigned int fwords, Also also) {
    const int p = blockIdx.y;
    const unsigned int q = blockIdx.x * MT_ROW_WG + threadIdx.x;
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
        accept = i >= 0 && (s == inf || b < __fmul_rn(ratio2, s)) && also(p, q, b, i);
    }
    const unsigned long long w = __ballot(accept);
    if ((threadIdx.x & 63) == 0 && q / 64 < fwords) flags[(size_t)p * fwords + q / 64] = w;
}

// ---- the guided passes ----

__device__ __forceinline__ double guided_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// The two-view section's coordinates of a point, exact; false: the point's octave is outside 0 .. 31
__device__ __forceinline__ bool guided_xy(const vslam_point& p, double& x, double& y) {
    if ((unsigned int)p.octave > 31u) return false;
    const double s = p.octave == 0 ? 0.5 : (double)(1u << (p.octave - 1));
    x = (double)((long long)p.col - (long long)p.padding) * s;
    y = (double)((long long)p.row - (long long)p.padding) * s;
    return true;
}

// The GuidedRow of a point at (x, y) under a fundamental matrix.  A query row: {a0, a1, a2, a0*a0 + a1*a1} with a = F x; a train
// row: {x', y', b0*b0, b1*b1} with b = F^T x'.  Per element that leaves  e = (x'*a0 + y'*a1) + a2;  e*e < max_dist2 * ((na + bb0) + bb1).
template <bool QUERY>
__device__ __forceinline__ GuidedRow guided_row_f(const double* F, double x, double y) {
    if (QUERY) {
        const double a0 = (F[0] * x + F[1] * y) + F[2], a1 = (F[3] * x + F[4] * y) + F[5], a2 = (F[6] * x + F[7] * y) + F[8];
        return GuidedRow{{a0, a1, a2, a0 * a0 + a1 * a1}};
    }
    const double b0 = (F[0] * x + F[3] * y) + F[6], b1 = (F[1] * x + F[4] * y) + F[7];
    return GuidedRow{{x, y, b0 * b0, b1 * b1}};
}

struct GuidedQn {  // the f32 side of a query row in LDS
    float norm;
    int octave;
};

// Query rows whose LDS reads the epilogue of guided_search keeps in flight together.  From the compiler's resource report:
// 1 -> 252 / 248 VGPRs (same_octave on / off), no scratch; 2 -> 256 with 4 spilled / 248; 4 -> 256 with 24 spilled / 256.
constexpr int GUIDED_ROWS_IN_FLIGHT = 1;

// The search of k_match_guided and k_match_guided_hf for query tile blockIdx.x, split blockIdx.y of pair p: the matcher's tiling
// and MFMA chain with one f64 predicate per (query, train) element in the epilogue, grouped exactly as the header writes it so
// that every operation rounds on its own.  KIND_H: the window around H x, dx = p0 - x'*p2; dy = p1 - y'*p2; dx*dx + dy*dy < L
// (seven f64 operations); else the epipolar band (nine).  What a lane knows about its 16 query rows beyond the running
// (best, second, index) lives in LDS, not in registers (the f64 coefficients alone would be 128 VGPRs): s_qa, one GuidedRow per
// query row of the tile, and s_qn {norm, octave}; the 32 lanes of a half read the same row, a broadcast.  The train tile's
// GuidedRows are staged with the tile (s_tc, flat: one f64 per thread).  An element that is not a candidate gets d2 = +inf
// before the selection, which is the header's "skipped".
template <bool SAME_OCT, bool KIND_H>
__device__ __forceinline__ void guided_search(const vslam_desc_sets& Q, const vslam_desc_sets& T, const float* __restrict__ qnorm,
                                              const float* __restrict__ tnorm, const GuidedRow* __restrict__ qrows,
                                              const GuidedRow* __restrict__ trows, double max_dist2, int nsplit, MatchPart* __restrict__ part, int p,
                                              unsigned int nq, unsigned int nt, float4* s_b, float* s_nb, int* s_tk, MatchPart* s_res, GuidedRow* s_qa,
                                              GuidedQn* s_qn, double* s_tc) {
    static_assert(MT_T * 4 == 256, "one f64 of the tile's GuidedRows per thread");
    const int split = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31, h = lane >> 5;
    const unsigned int qbase = blockIdx.x * MT_Q;
    const float inf = match_inf();

    float a[64];
    match_load_a(a, Q, p, min(qbase + wave * 32 + col, nq - 1), h);
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

    const unsigned int ntiles = (nt + MT_T - 1) / MT_T;
    float4 pf[8];
    float pnb = 0.0f;
    int ptk = 0;
    double ptc = 0.0;
    auto gload = [&](unsigned int tile) {
        match_tile_gload<SAME_OCT>(pf, pnb, ptk, T, tnorm, p, nt, tile, t);
        const unsigned int j = tile * MT_T + (t >> 2);
        ptc = j < nt ? trows[(size_t)p * T.cap + j].v[t & 3] : guided_nan();
    };

    const float4 *b0p = match_b_ptr(s_b, 0, col, h), *b1p = match_b_ptr(s_b, 1, col, h);
    unsigned int tile = split;
    if (tile < ntiles) gload(tile);
    while (tile < ntiles) {
        __syncthreads();  // the previous tile has been read (and, the first time, nothing yet: s_qa / s_qn are published by the next barrier)
        match_tile_lstore(pf, pnb, ptk, s_b, s_nb, s_tk, t);
        s_tc[t] = ptc;
        __syncthreads();
        const unsigned int next = tile + nsplit;
        if (next < ntiles) gload(next);  // in flight under the MFMAs
        f32x16 acc0, acc1;
        match_mfma_chain(a, b0p, b1p, acc0, acc1);
        // epilogue: this lane's train column of each block against its 16 query rows, ascending train index
        auto select = [&](const f32x16& acc, int blk) {
            const int tc = 32 * blk + col;
            const float nb = s_nb[tc];
            const int tk = s_tk[tc];
            const double xp = s_tc[4 * tc + 0], yp = s_tc[4 * tc + 1];
            const double bb0 = KIND_H ? 0.0 : s_tc[4 * tc + 2], bb1 = KIND_H ? 0.0 : s_tc[4 * tc + 3];
            const int j = (int)(tile * MT_T) + tc;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qr = wave * 32 + match_cd_row(r, h);
                const GuidedRow qa = s_qa[qr];
                const GuidedQn qn = s_qn[qr];
                bool candidate;
                if (KIND_H) {  // in window: qa = {p0, p1, p2, L}
                    const double dx = qa.v[0] - xp * qa.v[2], dy = qa.v[1] - yp * qa.v[2];
                    candidate = dx * dx + dy * dy < qa.v[3];
                } else {  // in band: qa = {a0, a1, a2, a0*a0 + a1*a1}
                    const double e = (xp * qa.v[0] + yp * qa.v[1]) + qa.v[2];
                    candidate = e * e < max_dist2 * ((qa.v[3] + bb0) + bb1);
                }
                const float s = acc[r];
                float d2 = (qn.norm + nb) - 2.0f * s;
                if (SAME_OCT && qn.octave != tk) d2 = inf;
                if (!candidate) d2 = inf;
                match_nn2_update(best, second, index, r, d2, j);
                // the scheduler may not pull the next rows' LDS reads up past this point: with all 16 rows' coefficients in flight
                // at once (160 registers) the kernel spills; GUIDED_ROWS_IN_FLIGHT rows' worth hides the read latency
                if (r % GUIDED_ROWS_IN_FLIGHT == GUIDED_ROWS_IN_FLIGHT - 1) __builtin_amdgcn_sched_barrier(0);
            }
        };
        select(acc0, 0);
        select(acc1, 1);
        tile = next;
    }
    match_finish(best, second, index, s_res, part, Q, p, nsplit, split, qbase, nq, t, wave, col, h);
}

}  // namespace vslam
