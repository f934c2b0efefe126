// Bundle adjustment (include/vslam.h, "bundle adjustment"): alternating Gauss-Newton over the tracks' points and the train cameras.
//   (k_chain_link and k_trk_next, through vslam::enqueue_chain_link and vslam::enqueue_trk_next, fill prev and next)
//   k_ba_init         : one lane per record: tracks_in -> tracks, point_info zeroed at the head slots of active tracks; the first
//                       lane of a pair's first workgroup: the camera T_j -> BaCam
//   k_ba_points       : step A, one lane per record.  A record that is not the head of an active track leaves at once.  A head
//                       walks its path with the ten sums in registers, solves, and walks it again under X_new; X is updated in
//                       place by the one lane that owns the track.  The cameras are read from the state through addresses
//                       that are the same in every lane of a wave (the lanes of a wave start in one pair and advance in step)
//   k_ba_cam_pass     : the hot path, grid = (blocks of 4096 rows, pairs), 256 lanes = the 256 slots of the ordered sum.  Per
//                       row the gathers - match record, refs, the head's row of tracks, the point record -, then membership,
//                       the residual, both Jacobian rows and all 29 sums in one walk (RR_ROW_SUMS, the refinement's text); the
//                       camera comes through blockIdx.y, so it is wave-uniform.  The tree is refit_tree<29>; the block's sums
//                       go to the scratch with plain stores.  Twice per sweep - the cameras, the candidates - and once at the end
//   k_ba_cam_step     : one lane per pair, after each pass: the block sums added left to right; after the cameras' pass STEP
//                       (RR_STEP_SOLVE: the 6 x 7 matrix in LDS) and the candidate; after the candidates' pass keep or drop;
//                       after the last pass the record of cams
//   k_ba_member_bits  : one lane per record: both sides' membership under the output, the wave's two ballot words
//   k_ba_points_final : one lane per record: a head's n_ok, status, canonical X and the rest of its point_info
// No floating-point atomics, no flags or fences between workgroups: kernel boundaries order everything.  A workgroup of the
// pass leaves before its first barrier or not at all (workgroup-uniform).  The arithmetic is the header's, operation for
// operation, under the rules of kernels_epipolar.hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_resect_refine_step.hip.h"
#include "kernels_tracks_views.hip.h"
#include "vslam_bundle_plan.h"

namespace vslam {

constexpr int BA_CUR = 0, BA_CAND = 1, BA_FINAL = 2;  // what a pass evaluated: the cameras, the candidates, the output

// The camera of view: T_j as kept so far, or the held camera (I, 0) for j < 0.
__device__ __forceinline__ void ba_load_cam(const BaCam* __restrict__ cams, int j, double (&W)[9], double (&w)[3]) {
    if (j < 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) W[k] = k % 4 == 0 ? 1.0 : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = 0.0;
    } else {
        const BaCam& c = cams[j];
#pragma unroll
        for (int k = 0; k < 9; ++k) W[k] = c.Wcur[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] = c.wcur[k];
    }
}

// The pair whose train camera is the query camera of pair j; -1: the held camera of a segment start.
__device__ __forceinline__ int ba_query_cam(const TrkIn& in, int j) { return j >= 1 && in.chain[j].linked ? j - 1 : -1; }

// h_j: the rows the heads of pair j + 1 may add to camera T_j.
__device__ __forceinline__ unsigned int ba_head_rows(const TrkIn& in, int j) {
    return j + 1 < in.n_pairs && in.chain[j + 1].linked ? g3_count(in.counts, j + 1, in.mcap) : 0u;
}

// EVALUATE-POINT of one view; JAC: with H and g.  H = {H00, H01, H02, H11, H12, H22}.
template <bool JAC>
__device__ __forceinline__ void ba_point_view(const double (&W)[9], const double (&w)[3], double u, double v, const double (&X)[3], double fx, double fy,
                                              double max_dist2, double (&H)[6], double (&g)[3], double& cost, unsigned int& n) {
    double Z[3];
    if (!rr_member(W, w, fx, fy, X[0], X[1], X[2], u, v, max_dist2, Z)) return;
    const double iz = 1.0 / Z[2];
    const double px = Z[0] * iz, py = Z[1] * iz;
    const double rx = (px - u) * fx, ry = (py - v) * fy;
    if (JAC) {
        const double sx = fx * iz, sy = fy * iz;
        double ax[3], ay[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) ax[k] = sx * (W[k] - px * W[6 + k]), ay[k] = sy * (W[3 + k] - py * W[6 + k]);
        int e = 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int c = k; c < 3; ++c, ++e) H[e] = H[e] + (ax[k] * ax[c] + ay[k] * ay[c]);
            g[k] = g[k] + (ax[k] * rx + ay[k] * ry);
        }
    }
    cost = cost + (rx * rx + ry * ry);
    n += 1;
}

// The views of the track headed by the live head (j0, i0) with indices (q, t), in order: f(W, w, u, v) per view.
template <class F>
__device__ __forceinline__ void ba_walk(const TrkIn& in, const vslam_pose_params& K, const BaCam* __restrict__ cams, const unsigned int* __restrict__ next,
                                        int j0, unsigned int i0, unsigned int q, unsigned int t, F f) {
    double W[9], w[3], u, v;
    int j = j0;
    unsigned int i = i0, tt = t;
    ba_load_cam(cams, ba_query_cam(in, j0), W, w);
    trk_pixel(in.frames[(size_t)j0 * in.pcap + q], K, u, v);
    f(W, w, u, v);
    for (;;) {
        const unsigned int b = trk_successor(in, next, j, i);
        if (b == TRK_NONE) break;
        ++j, i = b;
        const vslam_match rec = in.matches[(size_t)j * in.mcap + i];  // live: both indices address a point
        tt = (unsigned int)rec.train;
        ba_load_cam(cams, j - 1, W, w);
        trk_pixel(in.frames[(size_t)j * in.pcap + (unsigned int)rec.query], K, u, v);
        f(W, w, u, v);
    }
    ba_load_cam(cams, j, W, w);
    trk_pixel(in.frames[(size_t)(j + 1) * in.pcap + tt], K, u, v);
    f(W, w, u, v);
}

__device__ __forceinline__ bool ba_active(const vslam_track& row, unsigned int min_views) { return (row.status & 1u) && row.n_views >= min_views; }

// grid = (record blocks of 256, n_pairs).  tracks may be tracks_in.
__global__ __launch_bounds__(TRK_REC_WG) void k_ba_init(TrkIn in, vslam_bundle_params prm, const unsigned int* __restrict__ prev,
                                                         const unsigned int* __restrict__ next, const vslam_track* tracks_in,
                                                         const vslam_bundle_cam* __restrict__ cams_in, vslam_track* tracks,
                                                         vslam_bundle_point* __restrict__ info, BaCam* __restrict__ cams) {
    const int j = blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        BaCam s;
        s.valid = in.poses[j].best >= 0 ? 1 : 0;
        if (!s.valid) {
#pragma unroll
            for (int k = 0; k < 9; ++k) s.Wcur[k] = k % 4 == 0 ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s.wcur[k] = 0.0;
        } else if (cams_in) {
#pragma unroll
            for (int k = 0; k < 9; ++k) s.Wcur[k] = cams_in[j].W[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) s.wcur[k] = cams_in[j].w[k];
        } else {  // view L of the tracks section (the pixel of point 0 comes with it and is dropped)
            TrkView vw;
            trk_train_view(in, prm.K, j, 0u, vw);
#pragma unroll
            for (int k = 0; k < 9; ++k) s.Wcur[k] = vw.W[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) s.wcur[k] = vw.w[k];
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) s.Wcand[k] = s.Wcur[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) s.wcand[k] = s.wcur[k];
        s.cost_cur = s.cost_before = 0.0;
        s.n_cur = s.n_before = s.accepted = s.rejected = s.invalid = s.skipped = 0;
        s.has_cand = 0;
        cams[j] = s;
    }
    const unsigned int m = g3_count(in.counts, j, in.mcap);
    const size_t i = g3_record(blockIdx.x, TRK_REC_WG, threadIdx.x);
    if (i >= m) return;
    const size_t o = (size_t)j * in.mcap + i;
    const vslam_track row = tracks_in[o];
    if (tracks != tracks_in) tracks[o] = row;
    unsigned int q, t;
    if (info && ba_active(row, prm.min_views) && trk_live(in, j, i, q, t) && trk_head(in, prev, next, j, i, q))
        info[o] = vslam_bundle_point{0u, 0u, 0u, 0u, 0u, 0u, 0.0, 0.0};
}

// grid = (record blocks of 256, n_pairs): step A of sweep `sweep`.  info may be null.
__global__ __launch_bounds__(TRK_REC_WG) void k_ba_points(TrkIn in, vslam_bundle_params prm, const unsigned int* __restrict__ prev,
                                                           const unsigned int* __restrict__ next, const BaCam* __restrict__ cams, vslam_track* tracks,
                                                           vslam_bundle_point* __restrict__ info, unsigned int sweep) {
    const int j0 = blockIdx.y;
    const unsigned int m = g3_count(in.counts, j0, in.mcap);
    const size_t i0 = g3_record(blockIdx.x, TRK_REC_WG, threadIdx.x);
    if (i0 >= m) return;
    unsigned int q, t;
    if (!trk_live(in, j0, i0, q, t) || !trk_head(in, prev, next, j0, i0, q)) return;
    const size_t o = (size_t)j0 * in.mcap + i0;
    vslam_track* row = tracks + o;
    if (!ba_active(*row, prm.min_views)) return;
    const double fx = prm.K.fx, fy = prm.K.fy, max_dist2 = prm.max_dist2;
    const double X[3] = {row->X[0], row->X[1], row->X[2]};
    double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0}, cost = 0.0;
    unsigned int n = 0;
    ba_walk(in, prm.K, cams, next, j0, (unsigned int)i0, q, t,
            [&](const double (&W)[9], const double (&w)[3], double u, double v) { ba_point_view<true>(W, w, u, v, X, fx, fy, max_dist2, H, g, cost, n); });
    unsigned int accepted = 0, rejected = 0, invalid = 0, skipped = 0;
    if (n < 2) {
        skipped = 1;
    } else {
        const double c00 = H[3] * H[5] - H[4] * H[4], c01 = H[2] * H[4] - H[1] * H[5], c02 = H[1] * H[4] - H[2] * H[3];
        const double c11 = H[0] * H[5] - H[2] * H[2], c12 = H[1] * H[2] - H[0] * H[4], c22 = H[0] * H[3] - H[1] * H[1];
        const double det = (H[0] * c00 + H[1] * c01) + H[2] * c02;
        const double d0 = -(((c00 * g[0] + c01 * g[1]) + c02 * g[2]) / det), d1 = -(((c01 * g[0] + c11 * g[1]) + c12 * g[2]) / det),
                     d2 = -(((c02 * g[0] + c12 * g[1]) + c22 * g[2]) / det);
        if (!(det > 0.0 && det < __builtin_huge_val() && rr_finite(d0) && rr_finite(d1) && rr_finite(d2))) {
            invalid = 1;
        } else {
            const double Xn[3] = {X[0] + d0, X[1] + d1, X[2] + d2};
            double Hn[6], gn[3], cost_new = 0.0;  // (not touched without the Jacobian)
            unsigned int n_new = 0;
            ba_walk(in, prm.K, cams, next, j0, (unsigned int)i0, q, t, [&](const double (&W)[9], const double (&w)[3], double u, double v) {
                ba_point_view<false>(W, w, u, v, Xn, fx, fy, max_dist2, Hn, gn, cost_new, n_new);
            });
            if (n_new > n || (n_new == n && cost_new < cost)) {
                row->X[0] = Xn[0], row->X[1] = Xn[1], row->X[2] = Xn[2];
                accepted = 1;
            } else {
                rejected = 1;
            }
        }
    }
    if (info) {
        vslam_bundle_point pi = info[o];
        if (sweep == 0) pi.n_before = n, pi.cost_before = cost;
        pi.accepted += accepted, pi.rejected += rejected, pi.invalid += invalid, pi.skipped += skipped;
        info[o] = pi;
    }
}

// The row "one side of record i of pair jj" counts (header, step B): its indices and its point Y.
__device__ __forceinline__ bool ba_row(const TrkIn& in, const vslam_track_ref* __restrict__ refs, const vslam_track* tracks, unsigned int min_views, int jj,
                                       size_t i, bool need_head, unsigned int& q, unsigned int& t, double (&Y)[3]) {
    if (!trk_live(in, jj, i, q, t)) return false;
    const vslam_track_ref ref = refs[(size_t)jj * in.mcap + i];
    if (ref.pos > (unsigned int)jj || (need_head && ref.pos != 0u)) return false;
    const int jh = jj - (int)ref.pos;
    if (ref.head_record >= g3_count(in.counts, jh, in.mcap)) return false;
    const vslam_track* row = tracks + (size_t)jh * in.mcap + ref.head_record;
    if (!((row->status & 1u) && row->n_views >= min_views)) return false;
    Y[0] = row->X[0], Y[1] = row->X[1], Y[2] = row->X[2];
    return true;
}

// grid = (blocks of 4096 rows, n_pairs).  partial [n_pairs][sum_blocks][RR_SUMS]: H's upper triangle row-major, g, cost, n.
__global__ __launch_bounds__(REFIT_WG) void k_ba_cam_pass(TrkIn in, vslam_bundle_params prm, const vslam_track_ref* __restrict__ refs,
                                                           const vslam_track* __restrict__ tracks, const BaCam* __restrict__ cams, int which,
                                                           double* __restrict__ partial, unsigned int sum_blocks) {
    __shared__ double lds[RR_SUMS * 128];  // 29696 bytes
    const int j = blockIdx.y;
    const BaCam* st = cams + j;
    if (!st->valid || (which == BA_CAND && !st->has_cand)) return;
    const unsigned int m0 = g3_count(in.counts, j, in.mcap);
    const size_t n_rows = (size_t)m0 + ba_head_rows(in, j);
    const size_t first = (size_t)blockIdx.x * REFIT_BLOCK;
    if (first >= n_rows) return;
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = which == BA_CAND ? st->Wcand[k] : st->Wcur[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = which == BA_CAND ? st->wcand[k] : st->wcur[k];
    const double fx = prm.K.fx, fy = prm.K.fy, max_dist2 = prm.max_dist2;
    double s[RR_SUMS];
#pragma unroll
    for (int k = 0; k < (int)RR_SUMS; ++k) s[k] = 0.0;
#pragma unroll 1
    for (unsigned int k = 0; k < REFIT_PER_LANE; ++k) {
        const size_t r = first + (size_t)k * REFIT_WG + threadIdx.x;
        if (r < n_rows) {
            const bool train = r < m0;
            unsigned int iq, it;
            double Y[3];
            if (ba_row(in, refs, tracks, prm.min_views, train ? j : j + 1, train ? r : r - m0, !train, iq, it, Y)) {
                double u, v;
                trk_pixel(in.frames[(size_t)(j + 1) * in.pcap + (train ? it : iq)], prm.K, u, v);
                const double Y0 = Y[0], Y1 = Y[1], Y2 = Y[2];
                RR_ROW_SUMS(R, t, fx, fy, Y0, Y1, Y2, u, v, max_dist2, s);
            }
        }
    }
    refit_tree<(int)RR_SUMS>(s, lds);
    if (threadIdx.x == 0) {
        double* out = partial + ((size_t)j * sum_blocks + blockIdx.x) * RR_SUMS;
#pragma unroll
        for (int k = 0; k < (int)RR_SUMS; ++k) out[k] = s[k];
    }
}

// grid = (pair blocks of 64), one lane per pair, after the pass of the same `which`.
__global__ __launch_bounds__(RR_PAIR_WG) void k_ba_cam_step(TrkIn in, const double* __restrict__ partial, unsigned int sum_blocks, int which,
                                                             unsigned int sweep, unsigned int sweeps, BaCam* __restrict__ state,
                                                             vslam_bundle_cam* __restrict__ cams) {
    __shared__ double a[42][RR_PAIR_WG];  // the 6 x 7 matrix of STEP, element e of lane l at a[e][l]: 21504 bytes
    const int j = blockIdx.x * RR_PAIR_WG + threadIdx.x, l = threadIdx.x;
    if (j >= in.n_pairs) return;  // (no barrier below: every lane works on its own column of a)
    BaCam* st = state + j;
    if (st->valid && !(which == BA_CAND && !st->has_cand)) {
        // the camera's sums: ((B_0 + B_1) + B_2) + ...
        const size_t n_rows = (size_t)g3_count(in.counts, j, in.mcap) + ba_head_rows(in, j);
        const unsigned int nb = (unsigned int)((n_rows + REFIT_BLOCK - 1) / REFIT_BLOCK);
        const double* src = partial + (size_t)j * sum_blocks * RR_SUMS;
        double s[RR_SUMS];
#pragma unroll
        for (int k = 0; k < (int)RR_SUMS; ++k) s[k] = nb ? src[k] : 0.0;
        for (unsigned int b = 1; b < nb; ++b) {
#pragma unroll
            for (int k = 0; k < (int)RR_SUMS; ++k) s[k] = s[k] + src[(size_t)b * RR_SUMS + k];
        }
        const unsigned int n = (unsigned int)s[28];
        const double cost = s[27];
        if (which == BA_CAND) {  // step B.4
            if (n > st->n_cur || (n == st->n_cur && cost < st->cost_cur)) {
#pragma unroll
                for (int k = 0; k < 9; ++k) st->Wcur[k] = st->Wcand[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) st->wcur[k] = st->wcand[k];
                st->n_cur = n, st->cost_cur = cost;
                st->accepted += 1;
            } else {
                st->rejected += 1;
            }
            st->has_cand = 0;
        } else {
            st->n_cur = n, st->cost_cur = cost;
            if (which == BA_CUR) {
                if (sweep == 0) st->n_before = n, st->cost_before = cost;
                if (n < 6) {  // step B.2
                    st->skipped += 1;
                } else {  // step B.3
                    RR_STEP_SOLVE(a, l, s, st->Wcur, st->wcur);
                    if (ok) {
#pragma unroll
                        for (int k = 0; k < 9; ++k) st->Wcand[k] = Rn[k];
#pragma unroll
                        for (int k = 0; k < 3; ++k) st->wcand[k] = tn[k];
                        st->has_cand = 1;
                    } else {
                        st->invalid += 1;
                    }
                }
            }
        }
    }
    if (which == BA_FINAL) {
        vslam_bundle_cam out;
        if (st->valid) {
            double W[9], w[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) W[k] = st->Wcur[k], out.W[k] = rr_canonical(W[k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) w[k] = st->wcur[k], out.w[k] = rr_canonical(w[k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) out.C[k] = rr_canonical(-((W[k] * w[0] + W[3 + k] * w[1]) + W[6 + k] * w[2]));
            out.n_before = st->n_before, out.n_after = st->n_cur;
            out.accepted = st->accepted, out.rejected = st->rejected, out.invalid = st->invalid, out.skipped = st->skipped;
            out.cost_before = rr_canonical(st->cost_before), out.cost_after = rr_canonical(st->cost_cur);
        } else {
#pragma unroll
            for (int k = 0; k < 9; ++k) out.W[k] = k % 4 == 0 ? 1.0 : 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) out.w[k] = out.C[k] = 0.0;
            out.n_before = out.n_after = out.accepted = out.rejected = out.invalid = 0;
            out.skipped = sweeps;
            out.cost_before = out.cost_after = 0.0;
        }
        cams[j] = out;
    }
}

// grid = (record blocks of 256, n_pairs), after the last camera step and before k_ba_points_final (it reads the status bits
// tracks_in had): bits [n_pairs][2][fwords].
__global__ __launch_bounds__(TRK_REC_WG) void k_ba_member_bits(TrkIn in, vslam_bundle_params prm, const vslam_track_ref* __restrict__ refs,
                                                                const vslam_track* __restrict__ tracks, const BaCam* __restrict__ cams,
                                                                unsigned long long* __restrict__ bits) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(in.counts, j, in.mcap);
    const size_t i = g3_record(blockIdx.x, TRK_REC_WG, threadIdx.x);
    if (!g3_wave_has_record(i, m)) return;
    bool mq = false, mt = false;
    if (i < m) {
        unsigned int q, t;
        double Y[3];
        if (ba_row(in, refs, tracks, prm.min_views, j, i, false, q, t, Y)) {
            double W[9], w[3], u, v, Z[3];
            ba_load_cam(cams, ba_query_cam(in, j), W, w);
            trk_pixel(in.frames[(size_t)j * in.pcap + q], prm.K, u, v);
            mq = rr_member(W, w, prm.K.fx, prm.K.fy, Y[0], Y[1], Y[2], u, v, prm.max_dist2, Z);
            ba_load_cam(cams, j, W, w);
            trk_pixel(in.frames[(size_t)(j + 1) * in.pcap + t], prm.K, u, v);
            mt = rr_member(W, w, prm.K.fx, prm.K.fy, Y[0], Y[1], Y[2], u, v, prm.max_dist2, Z);
        }
    }
    const unsigned long long wq = __ballot(mq), wt = __ballot(mt);
    const bool store = g3_first_lane(threadIdx.x);
    g3_store_word(bits, (size_t)j * 2, in.fwords, i, store, wq);
    g3_store_word(bits, (size_t)j * 2 + 1, in.fwords, i, store, wt);
}

// grid = (record blocks of 256, n_pairs), the last launch: the head rows of active tracks get their output form.
__global__ __launch_bounds__(TRK_REC_WG) void k_ba_points_final(TrkIn in, vslam_bundle_params prm, const unsigned int* __restrict__ prev,
                                                                 const unsigned int* __restrict__ next, const BaCam* __restrict__ cams, vslam_track* tracks,
                                                                 vslam_bundle_point* __restrict__ info) {
    const int j0 = blockIdx.y;
    const unsigned int m = g3_count(in.counts, j0, in.mcap);
    const size_t i0 = g3_record(blockIdx.x, TRK_REC_WG, threadIdx.x);
    if (i0 >= m) return;
    unsigned int q, t;
    if (!trk_live(in, j0, i0, q, t) || !trk_head(in, prev, next, j0, i0, q)) return;
    const size_t o = (size_t)j0 * in.mcap + i0;
    vslam_track row = tracks[o];
    if (!ba_active(row, prm.min_views)) return;
    const double fx = prm.K.fx, fy = prm.K.fy, max_dist2 = prm.max_dist2;
    const double X[3] = {row.X[0], row.X[1], row.X[2]};
    double H[6], g[3], cost = 0.0;  // (not touched without the Jacobian)
    unsigned int n = 0;
    ba_walk(in, prm.K, cams, next, j0, (unsigned int)i0, q, t,
            [&](const double (&W)[9], const double (&w)[3], double u, double v) { ba_point_view<false>(W, w, u, v, X, fx, fy, max_dist2, H, g, cost, n); });
    const bool solved = row.det > 0.0 && row.det < __builtin_huge_val() && rr_finite(X[0]) && rr_finite(X[1]) && rr_finite(X[2]);
    const bool good = solved && n == row.n_views && row.n_views >= prm.min_views;
#pragma unroll
    for (int k = 0; k < 3; ++k) row.X[k] = rr_canonical(X[k]);
    row.n_ok = n;
    row.status = (solved ? 1u : 0u) | (good ? 2u : 0u);
    tracks[o] = row;
    if (info) {
        vslam_bundle_point pi = info[o];
        pi.n_after = n, pi.cost_after = rr_canonical(cost), pi.cost_before = rr_canonical(pi.cost_before);
        info[o] = pi;
    }
}

}  // namespace vslam
