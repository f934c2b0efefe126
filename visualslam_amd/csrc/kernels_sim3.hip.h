// Frame structure and loop alignment (include/vslam.h, "frame structure" and "loop alignment"): the trajectory's cameras and
// world points seen per frame, and a RANSAC Sim(3) per slot of a set-pair table between two frames' world points.
//   k_frame_index  : one lane per record of pair j: a live record does atomicMin(&index[j][query], i) - pair j is frame j's
//                    source whenever it is valid - and atomicMin(&index[j + 1][train], i) where pair j is frame j + 1's source;
//                    the table is preset to 0xffffffff, which is the -1 of its int32 entries.  A sibling of k_chain_link
//                    (kernels_chain.hip.h), not a shared body: that kernel fills one row per pair by train index only, and its
//                    unit's device code must not move
//   k_frame_cams   : one lane per frame: the chain record copied, or the train camera by the walk's two product rules
//   k_sim3_corr    : one lane per match record: step 1's test, the wave's ballot word of usable records, {b} for the compaction
//                    (kernels_compact.hip.h, EpipolarEntries), the links; workgroup (0, p) writes m_p
//   k_sim3_gather  : one lane per row of the dense list: b -> {X, Y, uq, vq, ut, vt, b}, step 1 again from the same inputs
//   k_sim3_models  : one lane per (slot, hypothesis): sample 3 correspondences, Horn's closed form; everything in registers
//   k_sim3_score   : the hot path, slots x hypotheses x correspondences, two reprojection tests each: one lane per hypothesis
//                    with Af, af, Ab, ab (24 f64) in registers, composed once from the hypothesis and the slot's two cameras;
//                    the workgroup walks correspondence tiles staged in LDS (every lane reads the same address: a broadcast);
//                    34 multiplications and 24 additions per correspondence; integer atomicAdd of the lane's count
//   k_sim3_select  : one workgroup per slot: ransac_select (kernels_estimate.hip.h) with a Sim3Model
//   k_sim3_flags   : one lane per match record: usable and an inlier of the winner, the wave's ballot word
// Kernel boundaries order everything: no flags or fences between workgroups, no floating-point atomics.  The arithmetic is the
// header's, operation for operation, under the rules of kernels_epipolar.hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_estimate.hip.h"
#include "kernels_geom3.hip.h"
#include "vslam_sim3_plan.h"

namespace vslam {

// ---- frame structure ----

struct FrameIn {
    const vslam_pose* poses;
    const vslam_match* matches;
    const unsigned int* counts;
    const unsigned long long* bits;
    const vslam_chain* chain;
    unsigned int mcap, fwords, pcap;
    int n_pairs;
};

// The trajectory section's LIVE rule for record i < m of pair j (chain_live of kernels_chain.hip.h, over FrameIn).
__device__ __forceinline__ bool frame_live(const FrameIn& in, int j, size_t i, unsigned int& q, unsigned int& t) {
    if (in.poses[j].best < 0) return false;
    if (!((in.bits[(size_t)j * in.fwords + (i >> 6)] >> (i & 63)) & 1ull)) return false;
    const vslam_match rec = in.matches[(size_t)j * in.mcap + i];
    q = (unsigned int)rec.query, t = (unsigned int)rec.train;
    return q < in.pcap && t < in.pcap;
}

// grid = (record blocks of 256, n_pairs).  index [n_pairs + 1][pcap] was preset to 0xffffffff.
__global__ __launch_bounds__(TWOVIEW_REC_WG) void k_frame_index(FrameIn in, unsigned int* __restrict__ index) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(in.counts, j, in.mcap);
    const size_t i = g3_record(blockIdx.x, TWOVIEW_REC_WG, threadIdx.x);
    if (i >= m || !in.chain[j].valid) return;  // (an invalid pair is no frame's source)
    unsigned int q, t;
    if (!frame_live(in, j, i, q, t)) return;
    atomicMin(&index[(size_t)j * in.pcap + q], (unsigned int)i);
    const bool next_has_own = j + 1 < in.n_pairs && in.chain[j + 1].valid;
    if (!next_has_own) atomicMin(&index[((size_t)j + 1) * in.pcap + t], (unsigned int)i);
}

// grid = (frame blocks of 64).
__global__ __launch_bounds__(FRAME_CAM_WG) void k_frame_cams(const vslam_pose* __restrict__ poses, const vslam_chain* __restrict__ chain, int n_pairs,
                                                              vslam_frame_cam* __restrict__ cams) {
    const size_t f = (size_t)blockIdx.x * FRAME_CAM_WG + threadIdx.x;
    if (f > (size_t)n_pairs) return;
    vslam_frame_cam out;
#pragma unroll
    for (int k = 0; k < 9; ++k) out.W[k] = 0.0;
    out.w[0] = out.w[1] = out.w[2] = 0.0;
    out.segment = out.pair = -1, out.side = 0, out.valid = 0;
    if (f < (size_t)n_pairs && chain[f].valid) {
        const vslam_chain& cf = chain[f];
#pragma unroll
        for (int k = 0; k < 9; ++k) out.W[k] = cf.W[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) out.w[k] = cf.w[k];
        out.segment = cf.segment, out.pair = (int)f, out.side = 0, out.valid = 1;
    } else if (f >= 1 && chain[f - 1].valid) {
        const vslam_chain& cp = chain[f - 1];
        const vslam_pose& P = poses[f - 1];
        const double s = cp.scale;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                out.W[3 * i + k] = pose_canonical((P.R[3 * i] * cp.W[k] + P.R[3 * i + 1] * cp.W[3 + k]) + P.R[3 * i + 2] * cp.W[6 + k]);
            out.w[i] = pose_canonical(((P.R[3 * i] * cp.w[0] + P.R[3 * i + 1] * cp.w[1]) + P.R[3 * i + 2] * cp.w[2]) + s * P.t[i]);
        }
        out.segment = cp.segment, out.pair = (int)f - 1, out.side = 1, out.valid = 1;
    }
    cams[f] = out;
}

// ---- loop alignment ----

struct Sim3SideIn {  // one vslam_sim3_side
    const vslam_frame_cam* cams;
    const int* index;
    const double* map;
    const vslam_point* points;
    unsigned int map_cap, pcap, ptcap, map_pairs, n_frames;
};
// What the record kernels need to know of one call's inputs.
struct Sim3In {
    Sim3SideIn q, t;
    const vslam_set_pair* pairs;
    const vslam_match* matches;
    const unsigned int* counts;
    unsigned int mcap;
    const unsigned long long* select;  // null: every record is selected
    unsigned int fwords;
    vslam_pose_params K;
};

__device__ __forceinline__ bool sim3_finite(double x) { return fabs(x) < __builtin_huge_val(); }

// Slot p's frames; false: the slot is empty.
__device__ __forceinline__ bool sim3_slot(const vslam_set_pair* pairs, int p, unsigned int nq, unsigned int nt, unsigned int& qs, unsigned int& ts) {
    const vslam_set_pair sp = pairs[p];
    qs = (unsigned int)sp.query_set, ts = (unsigned int)sp.train_set;
    return qs < nq && ts < nt;
}
// m_p.
__device__ __forceinline__ unsigned int sim3_count(const Sim3In& in, int p, unsigned int& qs, unsigned int& ts) {
    return sim3_slot(in.pairs, p, in.q.n_frames, in.t.n_frames, qs, ts) ? g3_count(in.counts, p, in.mcap) : 0u;
}

// One side of step 1 for feature k of frame f: the link, and - when the side's conditions hold - the world point and (u, v).
__device__ __forceinline__ bool sim3_side(const Sim3SideIn& s, const vslam_pose_params& K, unsigned int f, unsigned int k, int& link, double (&X)[3],
                                          double& u, double& v) {
    link = -1;
    if (k >= min(s.pcap, s.ptcap)) return false;
    link = s.index[(size_t)f * s.pcap + k];
    const vslam_frame_cam& cam = s.cams[f];
    if (!cam.valid || (unsigned int)cam.pair >= s.map_pairs) return false;
    if (link < 0 || (unsigned int)link >= s.map_cap) return false;
    const vslam_point pt = s.points[(size_t)f * s.ptcap + k];
    if ((unsigned int)pt.octave > 31u) return false;
    const double st = pt.octave == 0 ? 0.5 : (double)(1u << (pt.octave - 1));
    const double xp = (double)((long long)pt.col - (long long)pt.padding) * st;
    const double yp = (double)((long long)pt.row - (long long)pt.padding) * st;
    u = (xp - K.cx) / K.fx;
    v = (yp - K.cy) / K.fy;
    const double* src = s.map + ((size_t)(unsigned int)cam.pair * s.map_cap + (unsigned int)link) * 3;
    X[0] = src[0], X[1] = src[1], X[2] = src[2];
    return sim3_finite(X[0]) && sim3_finite(X[1]) && sim3_finite(X[2]);
}

// Step 1 of record b of slot p = (qs, ts); true: usable.  The links are set whatever the answer.
__device__ __forceinline__ bool sim3_correspondence(const Sim3In& in, int p, unsigned int qs, unsigned int ts, size_t b, Sim3Rec& o, int& lq, int& lt) {
    const vslam_match rec = in.matches[(size_t)p * in.mcap + b];
    const bool uq = sim3_side(in.q, in.K, qs, (unsigned int)rec.query, lq, o.X, o.uq, o.vq);
    const bool ut = sim3_side(in.t, in.K, ts, (unsigned int)rec.train, lt, o.Y, o.ut, o.vt);
    const bool sel = !in.select || ((in.select[(size_t)p * in.fwords + (b >> 6)] >> (b & 63)) & 1ull);
    return sel && uq && ut;
}

// grid = (record blocks of 256, n_pairs).  idx [n_pairs][mcap] gets {query = b}; uflags the ballot words that hold a record
// below m_p; mcount [n_pairs] gets m_p; links may be null.
__global__ __launch_bounds__(TWOVIEW_REC_WG) void k_sim3_corr(Sim3In in, vslam_match* __restrict__ idx, unsigned long long* __restrict__ uflags,
                                                               unsigned int* __restrict__ mcount, int* __restrict__ links) {
    const int p = blockIdx.y;
    unsigned int qs, ts;
    const unsigned int m = sim3_count(in, p, qs, ts);
    if (blockIdx.x == 0 && threadIdx.x == 0) mcount[p] = m;
    const size_t b = g3_record(blockIdx.x, TWOVIEW_REC_WG, threadIdx.x);
    if (!g3_wave_has_record(b, m)) return;
    bool use = false;
    if (b < m) {
        const size_t o = (size_t)p * in.mcap + b;
        Sim3Rec c;
        int lq, lt;
        use = sim3_correspondence(in, p, qs, ts, b, c, lq, lt);
        vslam_match e;
        e.query = (int)b, e.train = 0, e.dist2 = 0.0f;
        idx[o] = e;
        if (links) links[2 * o] = lq, links[2 * o + 1] = lt;
    }
    const unsigned long long w = __ballot(use);
    g3_store_word(uflags, p, in.fwords, b, g3_first_lane(threadIdx.x), w);
}

// grid = (record blocks of 256, n_pairs).  didx [n_pairs][mcap]: the compacted {b}; ncorr [n_pairs] their counts (0 for an
// empty slot: its m_p is 0).
__global__ __launch_bounds__(TWOVIEW_REC_WG) void k_sim3_gather(Sim3In in, const vslam_match* __restrict__ didx, const unsigned int* __restrict__ ncorr,
                                                                 vslam_sim3_corr* __restrict__ corr) {
    const int p = blockIdx.y;
    const unsigned int n = g3_count(ncorr, p, in.mcap);
    const size_t r = g3_record(blockIdx.x, TWOVIEW_REC_WG, threadIdx.x);
    if (r >= n) return;
    unsigned int qs, ts;
    (void)sim3_slot(in.pairs, p, in.q.n_frames, in.t.n_frames, qs, ts);  // (n > 0: not empty)
    const unsigned int b = (unsigned int)didx[(size_t)p * in.mcap + r].query;
    Sim3Rec c;
    int lq, lt;
    (void)sim3_correspondence(in, p, qs, ts, b, c, lq, lt);
    vslam_sim3_corr out;
#pragma unroll
    for (int k = 0; k < 3; ++k) out.X[k] = c.X[k], out.Y[k] = c.Y[k];
    out.uq = c.uq, out.vq = c.vq, out.ut = c.ut, out.vt = c.vt;
    out.b = b, out.reserved = 0;
    corr[(size_t)p * in.mcap + r] = out;
}

// Step 3 from the three sample points; false: invalid (s, R, t are not written).
__device__ __forceinline__ bool sim3_model(const double (&X)[3][3], const double (&Y)[3][3], double& s, double (&R)[9], double (&t)[3]) {
    double cX[3], cY[3], A[3][3], B[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        cX[k] = ((X[0][k] + X[1][k]) + X[2][k]) / 3.0;
        cY[k] = ((Y[0][k] + Y[1][k]) + Y[2][k]) / 3.0;
    }
    double na[3], nb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) A[i][k] = X[i][k] - cX[k], B[i][k] = Y[i][k] - cY[k];
        na[i] = (A[i][0] * A[i][0] + A[i][1] * A[i][1]) + A[i][2] * A[i][2];
        nb[i] = (B[i][0] * B[i][0] + B[i][1] * B[i][1]) + B[i][2] * B[i][2];
    }
    const double a2 = (na[0] + na[1]) + na[2], b2 = (nb[0] + nb[1]) + nb[2];
    if (!g3_finite_nonzero(a2) || !g3_finite_nonzero(b2)) return false;  // (sums of squares: never negative)
    const double sc = sqrt(b2 / a2), si = 1.0 / sc;
    double M[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[3 * r + c] = (B[0][r] * A[0][c] + B[1][r] * A[1][c]) + B[2][r] * A[2][c];
    double Rc[9], n[3];
    if (!g3_nearest_rotation(M, Rc, n)) return false;
    double tc[3];
    bool fin = sim3_finite(sc) && sim3_finite(si);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        tc[i] = cY[i] - sc * ((Rc[3 * i] * cX[0] + Rc[3 * i + 1] * cX[1]) + Rc[3 * i + 2] * cX[2]);
        fin &= sim3_finite(tc[i]);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) fin &= sim3_finite(Rc[i]);
    if (!fin) return false;
    s = sc;
#pragma unroll
    for (int i = 0; i < 9; ++i) R[i] = Rc[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = tc[i];
    return true;
}

// grid = (hypothesis blocks of 64, n_pairs), one wave; no LDS: the three sample indices and points are statically indexed.
__global__ __launch_bounds__(SIM3_MODEL_WG) void k_sim3_models(const vslam_sim3_corr* __restrict__ corr, const unsigned int* __restrict__ ncorr,
                                                                unsigned int mcap, unsigned int NH, unsigned int seed,
                                                                vslam_sim3_hyp* __restrict__ hyp) {
    const int p = blockIdx.y;
    const unsigned int h = blockIdx.x * SIM3_MODEL_WG + threadIdx.x;
    if (h >= NH) return;
    double s = 0.0, R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t[3] = {0, 0, 0};
    bool ok = false;
    const unsigned int m = g3_count(ncorr, p, mcap);
    if (m >= 3) {
        // 2. the sample
        const unsigned int base = epi_mix(epi_mix(seed + (unsigned int)p) + h);
        unsigned int i0 = 0, i1 = 0, i2 = 0;
        int n = 0;
        for (unsigned int d = 0; d < 64 && n < 3; ++d) {
            const unsigned int r = epi_mix(base + d);
            const unsigned int i = (unsigned int)(((unsigned long long)r * m) >> 32);
            const bool seen = (n > 0 && i0 == i) || (n > 1 && i1 == i);
            if (!seen) {
                if (n == 0) i0 = i;
                else if (n == 1) i1 = i;
                else i2 = i;
                ++n;
            }
        }
        if (n == 3) {
            const vslam_sim3_corr* src = corr + (size_t)p * mcap;
            const unsigned int si[3] = {i0, i1, i2};
            double X[3][3], Y[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const vslam_sim3_corr& c = src[si[i]];
#pragma unroll
                for (int k = 0; k < 3; ++k) X[i][k] = c.X[k], Y[i][k] = c.Y[k];
            }
            ok = sim3_model(X, Y, s, R, t);  // 3. (s, R, t stay 0 when it fails)
        }
    }
    vslam_sim3_hyp* out = hyp + (size_t)p * NH + h;
    out->s = s;
#pragma unroll
    for (int i = 0; i < 9; ++i) out->R[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) out->t[i] = t[i];
    out->inliers = 0;
    out->valid = ok ? 1 : 0;
}

// Step 4: (Af, af) and (Ab, ab) of (s, R, t) between the cameras (Wq, wq) and (Wt, wt).
struct Sim3Maps {
    double Af[9], af[3], Ab[9], ab[3];
};
__device__ __forceinline__ void sim3_compose(double s, const double (&R)[9], const double (&t)[3], const vslam_frame_cam& cq, const vslam_frame_cam& ct,
                                             Sim3Maps& o) {
    const double si = 1.0 / s;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double P = (ct.W[3 * i] * R[k] + ct.W[3 * i + 1] * R[3 + k]) + ct.W[3 * i + 2] * R[6 + k];
            o.Af[3 * i + k] = s * P;
            const double Q = (cq.W[3 * i] * R[3 * k] + cq.W[3 * i + 1] * R[3 * k + 1]) + cq.W[3 * i + 2] * R[3 * k + 2];
            o.Ab[3 * i + k] = si * Q;
        }
        o.af[i] = ((ct.W[3 * i] * t[0] + ct.W[3 * i + 1] * t[1]) + ct.W[3 * i + 2] * t[2]) + ct.w[i];
        o.ab[i] = cq.w[i] - ((o.Ab[3 * i] * t[0] + o.Ab[3 * i + 1] * t[1]) + o.Ab[3 * i + 2] * t[2]);
    }
}

// The resection section's step-6 test of the point P under (A, a) against (u, v); false for A = a = 0 (Z2 > 0 fails) and for a NaN.
__device__ __forceinline__ bool sim3_reproj(const double (&A)[9], const double (&a)[3], double fx, double fy, const double (&P)[3], double u, double v,
                                            double max_dist2) {
    const double Z0 = ((A[0] * P[0] + A[1] * P[1]) + A[2] * P[2]) + a[0];
    const double Z1 = ((A[3] * P[0] + A[4] * P[1]) + A[5] * P[2]) + a[1];
    const double Z2 = ((A[6] * P[0] + A[7] * P[1]) + A[8] * P[2]) + a[2];
    const double ex = (u * Z2 - Z0) * fx, ey = (v * Z2 - Z1) * fy;
    return Z2 > 0.0 && (ex * ex + ey * ey) < max_dist2 * (Z2 * Z2);
}
// Step 5.
__device__ __forceinline__ bool sim3_inlier(const Sim3Maps& m, double fx, double fy, const Sim3Rec& c, double max_dist2) {
    return sim3_reproj(m.Af, m.af, fx, fy, c.X, c.ut, c.vt, max_dist2) && sim3_reproj(m.Ab, m.ab, fx, fy, c.Y, c.uq, c.vq, max_dist2);
}

// grid = (hypothesis blocks of 256, nsplit, n_pairs).  Lane = hypothesis; the workgroup's correspondence tiles (tile index =
// blockIdx.y + k * nsplit) are staged in LDS, 80 bytes a record, and every lane walks them in step: the LDS address is the same
// in all lanes.  The lane's integer count goes into its hypothesis by atomicAdd: integer sums merge exactly in any order.  A
// slot without correspondences - every empty slot - leaves before anything is read through its table entry.
__global__ __launch_bounds__(EPI_SCORE_WG) void k_sim3_score(const vslam_sim3_corr* __restrict__ corr, const unsigned int* __restrict__ ncorr,
                                                              unsigned int mcap, unsigned int NH, const vslam_set_pair* __restrict__ pairs,
                                                              const vslam_frame_cam* __restrict__ qcams, const vslam_frame_cam* __restrict__ tcams,
                                                              double fx, double fy, double max_dist2, vslam_sim3_hyp* __restrict__ hyp) {
    __shared__ Sim3Rec tile[EPI_TILE];
    const int p = blockIdx.z;
    const unsigned int m = g3_count(ncorr, p, mcap);
    if (m == 0) return;  // block-uniform
    const unsigned int h = blockIdx.x * EPI_SCORE_WG + threadIdx.x;
    vslam_sim3_hyp* mine = hyp + (size_t)p * NH + min(h, NH - 1);
    Sim3Maps maps;
    {
        double R[9], t[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = mine->R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = mine->t[i];
        const vslam_set_pair sp = pairs[p];
        sim3_compose(mine->s, R, t, qcams[(unsigned int)sp.query_set], tcams[(unsigned int)sp.train_set], maps);
    }
    const bool counts = h < NH && mine->valid != 0;
    const vslam_sim3_corr* src = corr + (size_t)p * mcap;
    unsigned int count = 0;
    for (size_t t0 = (size_t)blockIdx.y * EPI_TILE; t0 < m; t0 += (size_t)gridDim.y * EPI_TILE) {  // block-uniform trip count
        const unsigned int n = (unsigned int)min((size_t)EPI_TILE, m - t0);
        __syncthreads();
        static_assert(EPI_TILE == EPI_SCORE_WG, "one correspondence per lane when a tile is staged");
        if (threadIdx.x < n) {
            const vslam_sim3_corr& c = src[t0 + threadIdx.x];
            tile[threadIdx.x] = Sim3Rec{{c.X[0], c.X[1], c.X[2]}, {c.Y[0], c.Y[1], c.Y[2]}, c.uq, c.vq, c.ut, c.vt};
        }
        __syncthreads();
        if (n == EPI_TILE) {
#pragma unroll 2
            for (unsigned int i = 0; i < EPI_TILE; ++i) count += sim3_inlier(maps, fx, fy, tile[i], max_dist2) ? 1u : 0u;
        } else {
            for (unsigned int i = 0; i < n; ++i) count += sim3_inlier(maps, fx, fy, tile[i], max_dist2) ? 1u : 0u;
        }
    }
    if (counts && count) atomicAdd(&mine->inliers, count);
}

// grid = (n_pairs)
__global__ __launch_bounds__(256) void k_sim3_select(const vslam_sim3_hyp* __restrict__ hyp, const unsigned int* __restrict__ mcount,
                                                      const unsigned int* __restrict__ ncorr, unsigned int mcap, unsigned int NH,
                                                      const vslam_set_pair* __restrict__ pairs, const vslam_frame_cam* __restrict__ qcams,
                                                      unsigned int nq, const vslam_frame_cam* __restrict__ tcams, unsigned int nt,
                                                      vslam_sim3* __restrict__ models) {
    const int p = blockIdx.x;
    ransac_select<Sim3Model>(hyp + (size_t)p * NH, NH, models + p, [&](vslam_sim3& out) {
        unsigned int qs, ts;
        const bool there = sim3_slot(pairs, p, nq, nt, qs, ts);
        out.n_matches = mcount[p];
        out.n_corr = g3_count(ncorr, p, mcap);
        out.query_segment = there ? qcams[qs].segment : -1;
        out.train_segment = there ? tcams[ts].segment : -1;
        out.reserved = 0;
    });
}

// grid = (record blocks of 256, n_pairs): bit b % 64 of word b / 64 = record b is usable and an inlier of the winner; the words
// that hold a record below m_p are written (all zero without a winner), the others left alone.
__global__ __launch_bounds__(TWOVIEW_REC_WG) void k_sim3_flags(Sim3In in, const vslam_sim3* __restrict__ models, double max_dist2,
                                                                unsigned long long* __restrict__ flags) {
    const int p = blockIdx.y;
    unsigned int qs, ts;
    const unsigned int m = sim3_count(in, p, qs, ts);
    const size_t b = g3_record(blockIdx.x, TWOVIEW_REC_WG, threadIdx.x);
    if (!g3_wave_has_record(b, m)) return;
    bool inl = false;
    if (b < m && models[p].best >= 0) {
        Sim3Rec c;
        int lq, lt;
        if (sim3_correspondence(in, p, qs, ts, b, c, lq, lt)) {
            double R[9], t[3];
#pragma unroll
            for (int i = 0; i < 9; ++i) R[i] = models[p].R[i];
#pragma unroll
            for (int i = 0; i < 3; ++i) t[i] = models[p].t[i];
            Sim3Maps maps;
            sim3_compose(models[p].s, R, t, in.q.cams[qs], in.t.cams[ts], maps);
            inl = sim3_inlier(maps, in.K.fx, in.K.fy, c, max_dist2);
        }
    }
    const unsigned long long w = __ballot(inl);
    g3_store_word(flags, p, in.fwords, b, g3_first_lane(threadIdx.x), w);
}

}  // namespace vslam
