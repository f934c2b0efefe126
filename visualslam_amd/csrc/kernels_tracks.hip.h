// Tracks (include/vslam.h, "tracks"): the records of consecutive pairs that saw one scene point, linked into a path, and the
// point triangulated from all of the path's views.
//   (k_chain_link, through vslam::enqueue_chain_link, fills prev [n_pairs - 1][point_cap]: step 1)
//   k_trk_next : one lane per record b of pairs >= 1: a live record of a linked pair whose a = prev[j - 1][query] exists does
//                atomicMin(&next[j - 1][a], b) on a uint32 table preset to 0xffffffff - the "lowest candidate" of step 2
//   k_trk_walk : the hot path, one lane per record.  A record that is not a head leaves at once.  A head walks its path twice:
//                once for the nine sums of step 3, which stay in registers, then - X known - once for the reprojection test of
//                step 5, writing refs as it goes.  Every step is one dependent gather chain: next[j][i], the match record,
//                the point record (24 bytes), and the pair's camera through addresses that are the same in every lane of a
//                wave (the lanes of a wave start in one pair and advance in step).  The wave's heads, good tracks and longest
//                track leave through ballot / popcount / a shuffle maximum and one integer atomic each
//   k_trk_rows : one lane per record: the rows and refs of the records that are not heads, and the wave's good_bits word
// Kernel boundaries order everything: no flags or fences between workgroups, no floating-point atomics.  The arithmetic is
// the header's, operation for operation, under the rules of kernels_epipolar.hip.h.  The record rules and the views are
// kernels_tracks_views.hip.h's: the bundle adjustment walks the same paths.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_tracks_views.hip.h"

namespace vslam {

// grid = (record blocks of 256, n_pairs - 1): block row y walks pair y + 1 and fills the table row of pair y.
__global__ __launch_bounds__(TRK_REC_WG) void k_trk_next(TrkIn in, const unsigned int* __restrict__ prev, unsigned int* __restrict__ next) {
    const int j = blockIdx.y + 1;
    const unsigned int m = g3_count(in.counts, j, in.mcap);
    const size_t i = g3_record(blockIdx.x, TRK_REC_WG, threadIdx.x);
    if (i >= m || !in.chain[j].linked) return;
    unsigned int q, t;
    if (!trk_live(in, j, i, q, t)) return;
    const unsigned int a = prev[(size_t)(j - 1) * in.pcap + q];  // a record below m_{j-1} <= match_cap, or none
    if (a != TRK_NONE) atomicMin(&next[(size_t)(j - 1) * in.mcap + a], (unsigned int)i);
}

// grid = (record blocks of 256, n_pairs).  summary [n_pairs] was zeroed; refs and summary may be null.  Only the rows of heads
// are written here (k_trk_rows writes the others), and the refs of the records on the heads' paths: every live record lies on
// exactly one path, so no two lanes write one ref.
__global__ __launch_bounds__(TRK_REC_WG) void k_trk_walk(TrkIn in, vslam_tracks_params prm, const unsigned int* __restrict__ prev,
                                                          const unsigned int* __restrict__ next, vslam_track* __restrict__ tracks,
                                                          vslam_track_ref* __restrict__ refs, vslam_track_summary* summary) {
    const int j0 = blockIdx.y;
    const unsigned int m = g3_count(in.counts, j0, in.mcap);
    const size_t i0 = g3_record(blockIdx.x, TRK_REC_WG, threadIdx.x);
    if (!g3_wave_has_record(i0, m)) return;
    bool head = false, good = false;
    unsigned int n_views = 0;
    unsigned int q, t;
    if (i0 < m && trk_live(in, j0, i0, q, t)) head = trk_head(in, prev, next, j0, i0, q);
    if (head) {
        // steps 2 and 3: the query view of every record from the head on, then the train view of the last
        double A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
        TrkView vw;
        int j = j0;
        unsigned int i = (unsigned int)i0, qq = q, tt = t;
        for (;;) {
            trk_query_view(in, prm.K, j, qq, vw);
            trk_accumulate(vw, A, g);
            ++n_views;
            const unsigned int b = trk_successor(in, next, j, i);
            if (b == TRK_NONE) break;
            ++j, i = b;
            const vslam_match rec = in.matches[(size_t)j * in.mcap + i];  // live: both indices address a point
            qq = (unsigned int)rec.query, tt = (unsigned int)rec.train;
        }
        trk_train_view(in, prm.K, j, tt, vw);
        trk_accumulate(vw, A, g);
        ++n_views;
        // step 4
        const double c00 = A[3] * A[5] - A[4] * A[4], c01 = A[2] * A[4] - A[1] * A[5], c02 = A[1] * A[4] - A[2] * A[3];
        const double c11 = A[0] * A[5] - A[2] * A[2], c12 = A[1] * A[2] - A[0] * A[4], c22 = A[0] * A[3] - A[1] * A[1];
        const double det = (A[0] * c00 + A[1] * c01) + A[2] * c02;
        const double X[3] = {((c00 * g[0] + c01 * g[1]) + c02 * g[2]) / det, ((c01 * g[0] + c11 * g[1]) + c12 * g[2]) / det,
                             ((c02 * g[0] + c12 * g[1]) + c22 * g[2]) / det};
        const double inf = __builtin_huge_val();
        const bool solved = det > 0.0 && det < inf && fabs(X[0]) < inf && fabs(X[1]) < inf && fabs(X[2]) < inf;
        // step 5: the same path again
        unsigned int n_ok = 0, pos = 0;
        j = j0, i = (unsigned int)i0, qq = q, tt = t;
        for (;;) {
            trk_query_view(in, prm.K, j, qq, vw);
            n_ok += trk_view_ok(vw, X, prm) ? 1u : 0u;
            if (refs) refs[(size_t)j * in.mcap + i] = vslam_track_ref{(unsigned int)i0, pos};
            const unsigned int b = trk_successor(in, next, j, i);
            if (b == TRK_NONE) break;
            ++j, ++pos, i = b;
            const vslam_match rec = in.matches[(size_t)j * in.mcap + i];
            qq = (unsigned int)rec.query, tt = (unsigned int)rec.train;
        }
        trk_train_view(in, prm.K, j, tt, vw);
        n_ok += trk_view_ok(vw, X, prm) ? 1u : 0u;
        good = solved && n_ok == n_views && n_views >= prm.min_views;
        vslam_track out;
#pragma unroll
        for (int k = 0; k < 3; ++k) out.X[k] = pose_canonical(X[k]);
        out.det = pose_canonical(det);
        out.n_views = n_views, out.n_ok = n_ok;
        out.status = (solved ? 1u : 0u) | (good ? 2u : 0u);
        out.reserved = 0;
        tracks[(size_t)j0 * in.mcap + i0] = out;
    }
    if (summary) {
        const unsigned int nh = __popcll(__ballot(head)), ng = __popcll(__ballot(good));
        unsigned int mv = n_views;
#pragma unroll
        for (int h = 32; h >= 1; h >>= 1) mv = max(mv, (unsigned int)__shfl_xor((int)mv, h));
        if (g3_first_lane(threadIdx.x) && nh) {
            atomicAdd(&summary[j0].n_heads, nh);
            if (ng) atomicAdd(&summary[j0].n_good, ng);
            atomicMax(&summary[j0].max_views, mv);
        }
    }
}

// grid = (record blocks of 256, n_pairs), after k_trk_walk: the rows of the records that are not heads, the refs of the
// records that are not live, and bit i % 64 of word i / 64 = record i heads a good track (refs and bits may be null).
__global__ __launch_bounds__(TRK_REC_WG) void k_trk_rows(TrkIn in, const unsigned int* __restrict__ prev, const unsigned int* __restrict__ next,
                                                          vslam_track* tracks, vslam_track_ref* __restrict__ refs,
                                                          unsigned long long* __restrict__ bits) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(in.counts, j, in.mcap);
    const size_t i = g3_record(blockIdx.x, TRK_REC_WG, threadIdx.x);
    if (!g3_wave_has_record(i, m)) return;
    bool good = false;
    if (i < m) {
        const size_t o = (size_t)j * in.mcap + i;
        unsigned int q, t;
        const bool live = trk_live(in, j, i, q, t);
        if (live && trk_head(in, prev, next, j, i, q)) {
            good = (tracks[o].status & 2u) != 0;
        } else {
            const double qnan = __longlong_as_double(TRK_QNAN);
            tracks[o] = vslam_track{{qnan, qnan, qnan}, qnan, 0u, 0u, 0u, 0u};
            if (refs && !live) refs[o] = vslam_track_ref{TRK_NONE, TRK_NONE};
        }
    }
    const unsigned long long w = __ballot(good);
    g3_store_word(bits, j, in.fwords, i, bits && g3_first_lane(threadIdx.x), w);
}

}  // namespace vslam
