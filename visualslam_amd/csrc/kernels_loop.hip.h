// The integer stages of loop verification (include/vslam.h, "loop verification"): table, gather and verdict.  Integers and copies
// only; kernel boundaries order everything, and no atomic is used at all.
//   k_loop_pairs   : one lane per slot of the nq * c table
//   k_pair_points  : grid = (ceil(match_cap / LP_WG), n_pairs), one lane per match record: two 24-byte gathers, three stores
//   k_loop_verdict : ONE workgroup of LP_WG lanes walks the frames in chunks of LP_WG, one frame per lane (its c slots in order, so
//                    a tie keeps the lower r); the list is compacted in frame order by a ballot and a prefix over the waves, the
//                    running total carried from chunk to chunk in a register every lane holds
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "vslam_loop_plan.h"  // pair_empty

namespace vslam {

// pairs [nq * c]
__global__ __launch_bounds__(LP_WG) void k_loop_pairs(const vslam_place_cand* __restrict__ candidates, const unsigned int* __restrict__ cand_counts,
                                                      unsigned int nq, unsigned int c, unsigned int db_first, unsigned int nd,
                                                      vslam_set_pair* __restrict__ pairs) {
    const size_t slot = (size_t)blockIdx.x * LP_WG + threadIdx.x;
    if (slot >= (size_t)nq * c) return;
    const unsigned int i = (unsigned int)(slot / c), r = (unsigned int)(slot % c);
    vslam_set_pair pr{-1, -1};
    if (r < min(cand_counts[i], c)) {
        const long long d = (long long)candidates[slot].frame - (long long)db_first;
        if (d >= 0 && d < (long long)nd) pr = vslam_set_pair{(int)i, (int)d};
    }
    pairs[slot] = pr;
}

// matches, qout, tout, local: [n_pairs][match_cap]
__global__ __launch_bounds__(LP_WG) void k_pair_points(const vslam_match* __restrict__ matches, const unsigned int* __restrict__ match_counts,
                                                       unsigned int match_cap, const vslam_set_pair* __restrict__ pairs, unsigned int n_query_sets,
                                                       unsigned int n_train_sets, const vslam_point* __restrict__ query_points, unsigned int query_cap,
                                                       const vslam_point* __restrict__ train_points, unsigned int train_cap,
                                                       vslam_point* __restrict__ qout, vslam_point* __restrict__ tout, vslam_match* __restrict__ local) {
    static_assert(sizeof(vslam_point) == 24, "a point is six 4-byte words");
    const int p = blockIdx.y;
    const unsigned int i = blockIdx.x * LP_WG + threadIdx.x;
    const vslam_set_pair pr = pairs[p];
    if (pair_empty(pr, n_query_sets, n_train_sets)) return;
    if (i >= min(match_counts[p], match_cap)) return;
    const size_t at = (size_t)p * match_cap + i;
    const vslam_match m = matches[at];
    // a point is six 4-byte words; an index past its list gives six words of all ones
    auto gather = [](const vslam_point* __restrict__ list, size_t set, unsigned int cap, unsigned int idx, vslam_point* __restrict__ dst) {
        const bool ok = idx < cap;
        const int* src = reinterpret_cast<const int*>(list + (ok ? set * cap + idx : 0));
        int* out = reinterpret_cast<int*>(dst);
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = ok ? src[k] : -1;
    };
    gather(query_points, (size_t)pr.query_set, query_cap, (unsigned int)m.query, qout + at);
    gather(train_points, (size_t)pr.train_set, train_cap, (unsigned int)m.train, tout + at);
    vslam_match l;
    l.query = (int)i;
    l.train = (int)i;
    l.dist2 = m.dist2;
    local[at] = l;
}

// grid = 1.  models, pairs: [nq * c]; loops [nq], loop_list [nq] and n_loops may each be null.
__global__ __launch_bounds__(LP_WG) void k_loop_verdict(const vslam_epipolar* __restrict__ models, const vslam_set_pair* __restrict__ pairs, unsigned int nq,
                                                        unsigned int c, unsigned int n_train_sets, vslam_loop_params P, vslam_loop* __restrict__ loops,
                                                        int* __restrict__ loop_list, unsigned int* __restrict__ n_loops) {
    __shared__ unsigned int s_wave[LP_WG / 64];
    const unsigned int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    unsigned int total = 0;  // loops of the frames before this chunk: the same in every lane
    for (unsigned int i0 = 0; i0 < nq; i0 += LP_WG) {
        const unsigned int i = i0 + t;
        bool has = false;
        if (i < nq) {
            vslam_loop L{(int)i, -1, -1, 0u, 0u};
            for (unsigned int r = 0; r < c; ++r) {
                const size_t p = (size_t)i * c + r;
                const vslam_set_pair pr = pairs[p];
                if (pair_empty(pr, nq, n_train_sets)) continue;
                const vslam_epipolar& m = models[p];
                const unsigned int ni = m.n_inliers, nm = m.n_matches;
                const bool verified = m.best >= 0 && ni >= P.min_inliers && (unsigned long long)ni * P.den >= (unsigned long long)P.num * nm;
                if (verified && (!has || ni > L.n_inliers)) {  // strictly more: equal counts keep the lower r
                    L = vslam_loop{pr.query_set, pr.train_set, (int)p, nm, ni};
                    has = true;
                }
            }
            if (loops) loops[i] = L;
        }
        const unsigned long long w = __ballot(has);
        if (lane == 0) s_wave[wave] = (unsigned int)__popcll(w);
        __syncthreads();
        unsigned int before = total, all = 0;
#pragma unroll
        for (unsigned int k = 0; k < LP_WG / 64; ++k) {
            before += k < wave ? s_wave[k] : 0u;
            all += s_wave[k];
        }
        if (has && loop_list) loop_list[before + (unsigned int)__popcll(w & ((1ull << lane) - 1ull))] = (int)i;
        total += all;
        __syncthreads();  // s_wave has been read
    }
    if (t == 0 && n_loops) *n_loops = total;
}

}  // namespace vslam
