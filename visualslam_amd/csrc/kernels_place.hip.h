// Loop candidates from word histograms (include/vslam.h, "place recognition", Place): unsigned integer arithmetic throughout,
// every sum in 64 bits, so no bit of any output depends on the order of anything.
//   k_place_df    : one lane per word: its document frequency over the db frames, and the weight
//   k_place_self  : one wave per frame (the query frames, then the db frames): the self-score
//   k_place_score : a workgroup owns PL_TILE x PL_TILE (query, db) frames, one pair per lane, and streams K through LDS in
//                   chunks of PL_KC words together with the weights; per four words a lane reads three 16-byte LDS operands
//                   (its query row's, shared by 16 lanes; its db row's; the weights', shared by all)
//   k_place_top   : one wave per query frame scans its row of scores; each lane keeps its best PL_MAX_C by the rank rule, then
//                   the wave takes the best head of all lanes c times.  The rank is a total order (the db index breaks every
//                   tie), so the merge is exact.
// Kernel boundaries order everything: no flags, no fences, no floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "vslam_place_plan.h"

namespace vslam {

__device__ __forceinline__ unsigned int place_saturate(unsigned long long v) { return v > 0x7fffffffull ? 0x7fffffffu : (unsigned int)v; }

// j is eligible for i
__device__ __forceinline__ bool place_eligible(unsigned int q_first, unsigned int i, unsigned int db_first, unsigned int j, unsigned int min_gap) {
    return (unsigned long long)db_first + j + min_gap <= (unsigned long long)q_first + i;
}

// a ranks before b; j: the db index (the frame ids are db_first + j, in the same order)
__device__ __forceinline__ bool place_before(unsigned int sa, unsigned int na, unsigned int ja, unsigned int sb, unsigned int nb, unsigned int jb) {
    const unsigned long long l = (unsigned long long)sa * nb, r = (unsigned long long)sb * na;
    return l > r || (l == r && ja < jb);
}

// grid = ceil(K / 256)
__global__ __launch_bounds__(256) void k_place_df(const unsigned int* __restrict__ hist_db, unsigned int nd, unsigned int K,
                                                  unsigned int* __restrict__ weights) {
    const unsigned int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    unsigned int df = 0;
    for (unsigned int j = 0; j < nd; ++j) df += hist_db[(size_t)j * K + k] > 0 ? 1u : 0u;
    weights[k] = df ? 32u - (unsigned int)__clz((int)(nd / df)) : 0u;
}

// grid = nq + nd, 64 lanes.  self_q [nq], self_db [nd].
__global__ __launch_bounds__(64) void k_place_self(const unsigned int* __restrict__ hist_q, unsigned int nq, const unsigned int* __restrict__ hist_db,
                                                   unsigned int K, const unsigned int* __restrict__ weights, unsigned int* __restrict__ self_q,
                                                   unsigned int* __restrict__ self_db) {
    const unsigned int b = blockIdx.x, lane = threadIdx.x;
    const unsigned int* row = b < nq ? hist_q + (size_t)b * K : hist_db + (size_t)(b - nq) * K;
    unsigned long long acc = 0;
    for (unsigned int k = lane; k < K; k += 64) acc += (unsigned long long)weights[k] * row[k];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int lo = __shfl_xor((unsigned int)acc, off), hi = __shfl_xor((unsigned int)(acc >> 32), off);
        acc += ((unsigned long long)hi << 32) | lo;
    }
    if (lane == 0) (b < nq ? self_q[b] : self_db[b - nq]) = place_saturate(acc);
}

constexpr unsigned int PL_LD = PL_KC + 4;  // words per LDS row: + 4 puts the 16 db rows that one 16-byte read cycle serves on all 64 banks

// grid = (ceil(nd / PL_TILE), ceil(nq / PL_TILE)), 256 lanes.  scores [nq][nd].  skip: a tile without an eligible pair returns at once.
__global__ __launch_bounds__(256) void k_place_score(const unsigned int* __restrict__ hist_q, unsigned int nq, unsigned int q_first,
                                                     const unsigned int* __restrict__ hist_db, unsigned int nd, unsigned int db_first, unsigned int K,
                                                     const unsigned int* __restrict__ weights, unsigned int min_gap, int skip,
                                                     unsigned int* __restrict__ scores) {
    __shared__ uint4 s_q[PL_TILE * PL_LD / 4];
    __shared__ uint4 s_d[PL_TILE * PL_LD / 4];
    __shared__ uint4 s_w[PL_KC / 4];
    const unsigned int t = threadIdx.x, ti = t >> 4, tj = t & 15;
    const unsigned int i0 = blockIdx.y * PL_TILE, j0 = blockIdx.x * PL_TILE;
    // the tile's most favourable pair: its last query frame and its first db frame
    if (skip && !place_eligible(q_first, min(i0 + PL_TILE - 1, nq - 1), db_first, j0, min_gap)) return;

    unsigned int* sq = reinterpret_cast<unsigned int*>(s_q);
    unsigned int* sd = reinterpret_cast<unsigned int*>(s_d);
    unsigned int* sw = reinterpret_cast<unsigned int*>(s_w);
    unsigned long long acc = 0;
    for (unsigned int k0 = 0; k0 < K; k0 += PL_KC) {
        __syncthreads();  // the previous chunk has been read
        // 2 x PL_TILE rows of PL_KC words, consecutive lanes on consecutive words; past a frame count or K: zeros
        for (unsigned int e = t; e < 2 * PL_TILE * PL_KC; e += 256) {
            const unsigned int r = e / PL_KC, k = e % PL_KC;
            unsigned int v = 0;
            if (k0 + k < K) {
                if (r < PL_TILE) {
                    if (i0 + r < nq) v = hist_q[(size_t)(i0 + r) * K + k0 + k];
                } else if (j0 + r - PL_TILE < nd) {
                    v = hist_db[(size_t)(j0 + r - PL_TILE) * K + k0 + k];
                }
            }
            (r < PL_TILE ? sq[r * PL_LD + k] : sd[(r - PL_TILE) * PL_LD + k]) = v;
        }
        if (t < PL_KC) sw[t] = k0 + t < K ? weights[k0 + t] : 0u;
        __syncthreads();
#pragma unroll 4
        for (unsigned int k = 0; k < PL_KC / 4; ++k) {
            const uint4 a = s_q[ti * (PL_LD / 4) + k], b = s_d[tj * (PL_LD / 4) + k], w = s_w[k];
            acc += (unsigned long long)w.x * min(a.x, b.x);
            acc += (unsigned long long)w.y * min(a.y, b.y);
            acc += (unsigned long long)w.z * min(a.z, b.z);
            acc += (unsigned long long)w.w * min(a.w, b.w);
        }
    }
    if (i0 + ti < nq && j0 + tj < nd) scores[(size_t)(i0 + ti) * nd + j0 + tj] = place_saturate(acc);
}

// grid = nq, 64 lanes.  candidates [nq][c] may be null; cand_counts [nq].
__global__ __launch_bounds__(64) void k_place_top(const unsigned int* __restrict__ scores, unsigned int nd, const unsigned int* __restrict__ self_q,
                                                  const unsigned int* __restrict__ self_db, unsigned int q_first, unsigned int db_first,
                                                  vslam_place_params P, vslam_place_cand* __restrict__ candidates,
                                                  unsigned int* __restrict__ cand_counts) {
    const unsigned int i = blockIdx.x, lane = threadIdx.x;
    constexpr unsigned int NONE = 0xffffffffu;  // an empty slot {0, 1, NONE} ranks after every candidate and before no slot
    unsigned int S[PL_MAX_C], N[PL_MAX_C], J[PL_MAX_C];
#pragma unroll
    for (unsigned int p = 0; p < PL_MAX_C; ++p) S[p] = 0, N[p] = 1, J[p] = NONE;
    const unsigned int sq = self_q[i];
    for (unsigned int j = lane; j < nd; j += 64) {
        if (!place_eligible(q_first, i, db_first, j, P.min_gap)) continue;
        unsigned int s = scores[(size_t)i * nd + j], n = max(sq, self_db[j]), jj = j;
        if (!(n > 0 && s >= P.min_score && (unsigned long long)s * P.den >= (unsigned long long)P.num * n)) continue;
        // insertion: the candidate sinks to its place, what it displaces sinks on
#pragma unroll
        for (unsigned int p = 0; p < PL_MAX_C; ++p) {
            if (place_before(s, n, jj, S[p], N[p], J[p])) {
                const unsigned int ts = S[p], tn = N[p], tj = J[p];
                S[p] = s, N[p] = n, J[p] = jj;
                s = ts, n = tn, jj = tj;
            }
        }
    }
    unsigned int count = 0;
    for (unsigned int r = 0; r < P.max_candidates; ++r) {
        unsigned int bs = S[0], bn = N[0], bj = J[0];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned int os = __shfl_xor(bs, off), on = __shfl_xor(bn, off), oj = __shfl_xor(bj, off);
            if (place_before(os, on, oj, bs, bn, bj)) bs = os, bn = on, bj = oj;
        }
        if (bj == NONE) break;  // (the same in every lane)
        if (lane == 0 && candidates) candidates[(size_t)i * P.max_candidates + r] = vslam_place_cand{(int)(db_first + bj), bs, bn};
        if (J[0] == bj) {  // the winner's lane takes its head off
#pragma unroll
            for (unsigned int p = 0; p + 1 < PL_MAX_C; ++p) S[p] = S[p + 1], N[p] = N[p + 1], J[p] = J[p + 1];
            S[PL_MAX_C - 1] = 0, N[PL_MAX_C - 1] = 1, J[PL_MAX_C - 1] = NONE;
        }
        ++count;
    }
    if (lane == 0) cand_counts[i] = count;
}

}  // namespace vslam
