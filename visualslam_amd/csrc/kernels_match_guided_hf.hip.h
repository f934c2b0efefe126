// Guided matching under H or F (include/vslam.h, "guided matching under H or F"): the guided pass of kernels_match_guided.hip.h
// with the candidate predicate chosen per pair - the epipolar band where the pair has an F, a window around H x where it has
// only an H, nothing where it has neither.  The kind is read on the device from the two model arrays (guided_kind); blockIdx.z
// (the rows kernel: blockIdx.y) is the pair, so the choice is uniform per workgroup.
//   k_guided_hf_rows  : one thread per row, one 32-byte GuidedRow per row.  Kind F: k_guided_rows' two records, operation for
//                       operation.  Kind H, query row: {p0, p1, p2, L} with p = H x and L = max_transfer2 * (p2*p2), NaN in
//                       every field when the row is not trusted or p2 > 0 is false; train row: {x', y', 0, 0}, NaN when not
//                       trusted.  Kind NONE: NaN.  Per element that leaves, under H,
//                       dx = p0 - x'*p2;  dy = p1 - y'*p2;  dx*dx + dy*dy < L  - seven f64 operations against the band's nine.
//   k_match_guided_hf : k_match_guided, statement for statement (tiling, MFMA chain, LDS image, selection, merge of the lanes),
//                       with the element predicate a template parameter.  A call launches the F form when it has epipolar
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

// grid = (ceil(cap / GUIDED_ROW_WG), pairs); rows [pair][S.cap]
template <bool QUERY>
__global__ __launch_bounds__(GUIDED_ROW_WG) void k_guided_hf_rows(const vslam_desc_sets S, const vslam_epipolar* __restrict__ emodels,
                                                                  const vslam_homography* __restrict__ hmodels, double max_transfer2,
                                                                  GuidedRow* __restrict__ rows) {
    const int p = blockIdx.y;
    const unsigned int r = blockIdx.x * GUIDED_ROW_WG + threadIdx.x;
    if (r >= min(S.counts[p], S.cap)) return;
    const double nan = guided_nan();
    GuidedRow out{{nan, nan, nan, nan}};
    const int kind = guided_kind(emodels, hmodels, p);
    double x, y;
    if (kind != GUIDED_KIND_NONE && guided_xy(S.points[(size_t)p * S.cap + r], x, y)) {
        if (kind == GUIDED_KIND_F) {
            const double* F = emodels[p].F;
            if (QUERY) {
                const double a0 = (F[0] * x + F[1] * y) + F[2], a1 = (F[3] * x + F[4] * y) + F[5], a2 = (F[6] * x + F[7] * y) + F[8];
                out = GuidedRow{{a0, a1, a2, a0 * a0 + a1 * a1}};
            } else {
                const double b0 = (F[0] * x + F[3] * y) + F[6], b1 = (F[1] * x + F[4] * y) + F[7];
                out = GuidedRow{{x, y, b0 * b0, b1 * b1}};
            }
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
__global__ __launch_bounds__(GUIDED_ROW_WG) void k_guided_hf_kinds(const vslam_epipolar* __restrict__ emodels, const vslam_homography* __restrict__ hmodels,
                                                                   int n_pairs, unsigned int* __restrict__ list, unsigned int* __restrict__ count) {
    __shared__ unsigned int s_n[3][GUIDED_ROW_WG];  // per thread: F, H, NONE pairs of its stretch, then their offsets
    const int t = threadIdx.x, per = (n_pairs + GUIDED_ROW_WG - 1) / GUIDED_ROW_WG;
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

// Query rows whose LDS reads the epilogue keeps in flight together: k_match_guided's choice (GUIDED_ROWS_IN_FLIGHT), for its reason.
constexpr int GUIDED_HF_ROWS_IN_FLIGHT = 1;

// grid = (ceil(Q.cap / MT_Q), nsplit, pairs).  part: [pair][split][Q.cap].  The MFMA chain, the LDS image of a train tile and the
// C / D map are k_match_nn2's (kernels_match.hip.h); everything but the first lines and the predicate is k_match_guided.
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
    const int split = blockIdx.y, t = threadIdx.x, lane = t & 63, wave = t >> 6, col = lane & 31, h = lane >> 5;
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
            const double xp = s_tc[4 * tc + 0], yp = s_tc[4 * tc + 1];
            const double bb0 = KIND_H ? 0.0 : s_tc[4 * tc + 2], bb1 = KIND_H ? 0.0 : s_tc[4 * tc + 3];
            const int j = (int)(tile * MT_T) + tc;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int qr = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
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
                const bool lt = d2 < best[r];
                const float s2 = d2 < second[r] ? d2 : second[r];
                second[r] = lt ? best[r] : s2;
                index[r] = lt ? j : index[r];
                best[r] = lt ? d2 : best[r];
                // (as k_match_guided) the scheduler may not pull the next rows' LDS reads up past this point
                if (r % GUIDED_HF_ROWS_IN_FLIGHT == GUIDED_HF_ROWS_IN_FLIGHT - 1) __builtin_amdgcn_sched_barrier(0);
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

}  // namespace vslam
