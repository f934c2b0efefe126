// What the kernels of the tracks step (kernels_tracks.hip.h) and of the bundle adjustment (kernels_bundle.hip.h) share, each
// stated once: the call's input lists, the LIVE and HEAD rules, a view's pixel and camera, steps 3 and 5 of one view and the
// successor on a path (include/vslam.h, "tracks").  Device functions only - no kernel -, so two translation units include it.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_geom3.hip.h"
#include "vslam_tracks_plan.h"

namespace vslam {

constexpr unsigned int TRK_NONE = 0xffffffffu;  // a table entry no record wrote (the memset's bytes); both fields of the ref of a record that is not live
constexpr long long TRK_QNAN = 0x7ff8000000000000ll;

// What the kernels need to know of one call's input lists.
struct TrkIn {
    const vslam_pose* poses;
    const vslam_match* matches;
    const unsigned int* counts;
    const unsigned long long* bits;
    const vslam_chain* chain;
    const vslam_point* frames;
    unsigned int mcap, fwords, pcap;
    int n_pairs;
};

// The trajectory section's LIVE rule for record i < m of pair j (kernels_chain.hip.h states it for its own input struct).
// q, t: the record's indices, set when live.
__device__ __forceinline__ bool trk_live(const TrkIn& in, int j, size_t i, unsigned int& q, unsigned int& t) {
    if (in.poses[j].best < 0) return false;
    if (!((in.bits[(size_t)j * in.fwords + (i >> 6)] >> (i & 63)) & 1ull)) return false;
    const vslam_match rec = in.matches[(size_t)j * in.mcap + i];
    q = (unsigned int)rec.query, t = (unsigned int)rec.train;
    return q < in.pcap && t < in.pcap;
}

// The live record i of pair j, query index q, is a head: it continues nothing (step 2).
__device__ __forceinline__ bool trk_head(const TrkIn& in, const unsigned int* __restrict__ prev, const unsigned int* __restrict__ next, int j, size_t i,
                                         unsigned int q) {
    if (j == 0 || !in.chain[j].linked) return true;
    const unsigned int a = prev[(size_t)(j - 1) * in.pcap + q];
    return a == TRK_NONE || next[(size_t)(j - 1) * in.mcap + a] != (unsigned int)i;
}

// One view (step 2): its camera, its centre and its calibrated pixel.
struct TrkView {
    double W[9], w[3], C[3], u, v;
};

// (u, v) of point record p: the exact coordinate (two-view geometry section), NaN for an octave outside 0 .. 31.
__device__ __forceinline__ void trk_pixel(const vslam_point& p, const vslam_pose_params& K, double& u, double& v) {
    double x = __longlong_as_double(TRK_QNAN), y = x;
    if ((unsigned int)p.octave <= 31u) {
        const double s = p.octave == 0 ? 0.5 : (double)(1u << (p.octave - 1));
        x = (double)((long long)p.col - (long long)p.padding) * s;
        y = (double)((long long)p.row - (long long)p.padding) * s;
    }
    u = (x - K.cx) / K.fx, v = (y - K.cy) / K.fy;
}

// The query view of a record of pair j with query index q.
__device__ __forceinline__ void trk_query_view(const TrkIn& in, const vslam_pose_params& K, int j, unsigned int q, TrkView& o) {
    const vslam_chain& cj = in.chain[j];
#pragma unroll
    for (int k = 0; k < 9; ++k) o.W[k] = cj.W[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) o.w[k] = cj.w[k], o.C[k] = cj.C[k];
    trk_pixel(in.frames[(size_t)j * in.pcap + q], K, o.u, o.v);
}

// The train view of a record of pair j with train index t: the camera (R W, R w + s t) by the trajectory's product rules.
__device__ __forceinline__ void trk_train_view(const TrkIn& in, const vslam_pose_params& K, int j, unsigned int t, TrkView& o) {
    const vslam_chain& cj = in.chain[j];
    const vslam_pose& pj = in.poses[j];
    const double s = cj.scale;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double r0 = pj.R[3 * i], r1 = pj.R[3 * i + 1], r2 = pj.R[3 * i + 2];
#pragma unroll
        for (int k = 0; k < 3; ++k) o.W[3 * i + k] = (r0 * cj.W[k] + r1 * cj.W[3 + k]) + r2 * cj.W[6 + k];
        o.w[i] = ((r0 * cj.w[0] + r1 * cj.w[1]) + r2 * cj.w[2]) + s * pj.t[i];
        o.C[i] = cj.Ct[i];
    }
    trk_pixel(in.frames[(size_t)(j + 1) * in.pcap + t], K, o.u, o.v);
}

// Step 3 of one view: A = {A00, A01, A02, A11, A12, A22}, g.
__device__ __forceinline__ void trk_accumulate(const TrkView& vw, double (&A)[6], double (&g)[3]) {
    const double d0 = (vw.W[0] * vw.u + vw.W[3] * vw.v) + vw.W[6], d1 = (vw.W[1] * vw.u + vw.W[4] * vw.v) + vw.W[7],
                 d2 = (vw.W[2] * vw.u + vw.W[5] * vw.v) + vw.W[8];
    const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
    const double e0 = d0 / dd, e1 = d1 / dd, e2 = d2 / dd;
    const double P00 = 1.0 - e0 * d0, P01 = 0.0 - e0 * d1, P02 = 0.0 - e0 * d2, P11 = 1.0 - e1 * d1, P12 = 0.0 - e1 * d2, P22 = 1.0 - e2 * d2;
    A[0] = A[0] + P00, A[1] = A[1] + P01, A[2] = A[2] + P02, A[3] = A[3] + P11, A[4] = A[4] + P12, A[5] = A[5] + P22;
    g[0] = g[0] + ((P00 * vw.C[0] + P01 * vw.C[1]) + P02 * vw.C[2]);
    g[1] = g[1] + ((P01 * vw.C[0] + P11 * vw.C[1]) + P12 * vw.C[2]);
    g[2] = g[2] + ((P02 * vw.C[0] + P12 * vw.C[1]) + P22 * vw.C[2]);
}

// Step 5 of one view.
__device__ __forceinline__ bool trk_view_ok(const TrkView& vw, const double (&X)[3], const vslam_tracks_params& prm) {
    const double Z0 = ((vw.W[0] * X[0] + vw.W[1] * X[1]) + vw.W[2] * X[2]) + vw.w[0];
    const double Z1 = ((vw.W[3] * X[0] + vw.W[4] * X[1]) + vw.W[5] * X[2]) + vw.w[1];
    const double Z2 = ((vw.W[6] * X[0] + vw.W[7] * X[1]) + vw.W[8] * X[2]) + vw.w[2];
    const double ex = (vw.u * Z2 - Z0) * prm.K.fx, ey = (vw.v * Z2 - Z1) * prm.K.fy;
    return Z2 > 0.0 && (ex * ex + ey * ey) < prm.max_dist2 * (Z2 * Z2);
}

// The record after (j, i) on its track, or TRK_NONE (the table has a row for every pair but the last).
__device__ __forceinline__ unsigned int trk_successor(const TrkIn& in, const unsigned int* __restrict__ next, int j, unsigned int i) {
    return j + 1 < in.n_pairs ? next[(size_t)j * in.mcap + i] : TRK_NONE;
}

}  // namespace vslam
