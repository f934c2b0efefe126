// Trajectory (include/vslam.h, "trajectory"): the poses and points vslam_pose_dev wrote for consecutive pairs, chained with
// the recovered scale into one world frame.
//   k_chain_link   : one lane per record of pair j - 1: a live record does atomicMin(&prev[j][train], i) on a uint32 table
//                    preset to 0xffffffff - an integer minimum is the same in any order: the "lowest i" of step 1
//   k_chain_ratio  : one lane per record of pair j: the linked record a = prev[j][query], one 24-byte gather from
//                    points[j - 1], the pair's (R, t) through addresses that are the same in every lane, r = |R X + t| / |Z|
//                    (step 2); the uint64 key of a usable r - or all ones - goes to the key scratch, the wave's usable count
//                    out through ballot + popcount and one integer atomicAdd
//   k_chain_median : one workgroup per pair, nothing shared between workgroups: a radix select over the pair's keys, most
//                    significant digit first, eight passes of eight bits - a 256-bin histogram in LDS by integer LDS
//                    atomics, a scan that finds the digit holding the wanted rank, the prefix narrowed.  Integers only:
//                    positive finite doubles order as their bit patterns, so the result is the multiset's (step 3)
//   k_chain_walk   : one lane, sequential over the pairs (step 4): not the hot path
//   k_chain_map    : one lane per record: the pair's W, w, scale wave-uniform, 24 bytes read and 24 written (step 5)
// Kernel boundaries order everything: no flags or fences between workgroups, no floating-point atomics.  The arithmetic is
// the header's, operation for operation, under the rules of kernels_epipolar.hip.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_geom3.hip.h"
#include "vslam_chain_plan.h"

namespace vslam {

constexpr unsigned int CHAIN_NO_LINK = 0xffffffffu;        // a link-table entry no live record wrote (the memset's bytes)
constexpr unsigned long long CHAIN_NO_KEY = ~0ull;         // the key of a record without a usable ratio
constexpr long long CHAIN_QNAN = 0x7ff8000000000000ll;

// What the kernels need to know of one call's input lists.
struct ChainIn {
    const vslam_pose* poses;
    const vslam_match* matches;
    const unsigned int* counts;
    const double* points;
    const unsigned long long* bits;
    unsigned int mcap, fwords, pcap;
};

// Record i < m of pair j is live: the pair has a winner (wave-uniform), the record is in front under it, and both of its
// indices address a point.  q, t: its indices, set when live.
__device__ __forceinline__ bool chain_live(const ChainIn& in, int j, size_t i, unsigned int& q, unsigned int& t) {
    if (in.poses[j].best < 0) return false;
    if (!((in.bits[(size_t)j * in.fwords + (i >> 6)] >> (i & 63)) & 1ull)) return false;
    const vslam_match rec = in.matches[(size_t)j * in.mcap + i];
    q = (unsigned int)rec.query, t = (unsigned int)rec.train;
    return q < in.pcap && t < in.pcap;
}

// y = (M v) + s * t, row by row, left to right: the product rule of steps 2 and 4 (s * t_i is t_i itself for s == 1).
__device__ __forceinline__ void chain_apply(const double (&M)[9], const double (&v)[3], double s, const double (&t)[3], double (&y)[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) y[i] = ((M[3 * i] * v[0] + M[3 * i + 1] * v[1]) + M[3 * i + 2] * v[2]) + s * t[i];
}

// grid = (record blocks of 256, n_pairs - 1): block row y walks pair y and fills the table row of pair y + 1.
__global__ __launch_bounds__(CHAIN_REC_WG) void k_chain_link(ChainIn in, unsigned int* __restrict__ prev) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(in.counts, j, in.mcap);
    const size_t i = g3_record(blockIdx.x, CHAIN_REC_WG, threadIdx.x);
    if (i >= m) return;
    unsigned int q, t;
    if (chain_live(in, j, i, q, t)) atomicMin(&prev[(size_t)j * in.pcap + t], (unsigned int)i);
}

// grid = (record blocks of 256, n_pairs).  keys [n_pairs - 1][mcap] and prev [n_pairs - 1][pcap] have no row for pair 0, which
// has no links; usable [n_pairs] was zeroed.  links and ratios may be null.
__global__ __launch_bounds__(CHAIN_REC_WG) void k_chain_ratio(ChainIn in, const unsigned int* __restrict__ prev, unsigned long long* __restrict__ keys,
                                                               unsigned int* usable, int* __restrict__ links, double* __restrict__ ratios) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(in.counts, j, in.mcap);
    const size_t i = g3_record(blockIdx.x, CHAIN_REC_WG, threadIdx.x);
    if (!g3_wave_has_record(i, m)) return;
    bool use = false;
    if (i < m) {
        int a = -1;
        double r = __longlong_as_double(CHAIN_QNAN);
        unsigned int q, t;
        if (j >= 1 && chain_live(in, j, i, q, t)) {
            const unsigned int p = prev[(size_t)(j - 1) * in.pcap + q];
            if (p != CHAIN_NO_LINK) {
                a = (int)p;
                const double* Xp = in.points + ((size_t)(j - 1) * in.mcap + p) * 3;
                const double* Zp = in.points + ((size_t)j * in.mcap + i) * 3;
                const vslam_pose& P = in.poses[j - 1];
                double R[9], tt[3], Y[3];
#pragma unroll
                for (int k = 0; k < 9; ++k) R[k] = P.R[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) tt[k] = P.t[k];
                const double X[3] = {Xp[0], Xp[1], Xp[2]};
                chain_apply(R, X, 1.0, tt, Y);
                const double dY = sqrt((Y[0] * Y[0] + Y[1] * Y[1]) + Y[2] * Y[2]);
                const double dZ = sqrt((Zp[0] * Zp[0] + Zp[1] * Zp[1]) + Zp[2] * Zp[2]);
                r = dY / dZ;
                use = r > 0.0 && r < __builtin_huge_val();
            }
        }
        const size_t o = (size_t)j * in.mcap + i;
        if (j >= 1) keys[(size_t)(j - 1) * in.mcap + i] = use ? (unsigned long long)__double_as_longlong(r) : CHAIN_NO_KEY;
        if (links) links[o] = a;
        if (ratios) ratios[o] = pose_canonical(r);
    }
    const unsigned int c = __popcll(__ballot(use));
    if (g3_first_lane(threadIdx.x) && c) atomicAdd(&usable[j], c);
}

// grid = (n_pairs - 1): workgroup x selects the median of pair x + 1 from keys row x.  One lane per radix bin.
__global__ __launch_bounds__(CHAIN_MEDIAN_WG) void k_chain_median(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ counts,
                                                                   unsigned int mcap, const unsigned int* __restrict__ usable, double* __restrict__ median) {
    __shared__ unsigned int hist[CHAIN_MEDIAN_WG], scan[2][CHAIN_MEDIAN_WG], sel_digit, sel_rank;
    const int j = blockIdx.x + 1;
    const unsigned int tid = threadIdx.x;
    const unsigned int n = usable[j];
    if (n == 0) {  // block-uniform
        if (tid == 0) median[j] = 0.0;
        return;
    }
    const size_t m = g3_count(counts, j, mcap);
    const unsigned long long* kj = keys + (size_t)(j - 1) * mcap;
    unsigned long long prefix = 0;
    unsigned int rank = (n - 1) >> 1;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        const unsigned long long above = pass == 0 ? 0ull : ~0ull << (shift + 8);  // the digits already decided
        hist[tid] = 0;
        __syncthreads();
        for (size_t i = tid; i < m; i += CHAIN_MEDIAN_WG) {
            const unsigned long long k = kj[i];
            if (k != CHAIN_NO_KEY && (k & above) == prefix) atomicAdd(&hist[(unsigned int)(k >> shift) & 255u], 1u);
        }
        __syncthreads();
        // inclusive scan of the 256 bins, one lane each
        const unsigned int h = hist[tid];
        scan[0][tid] = h;
        __syncthreads();
        int src = 0;
#pragma unroll
        for (unsigned int off = 1; off < CHAIN_MEDIAN_WG; off <<= 1) {
            const unsigned int v = scan[src][tid] + (tid >= off ? scan[src][tid - off] : 0u);
            scan[src ^ 1][tid] = v;
            __syncthreads();
            src ^= 1;
        }
        const unsigned int incl = scan[src][tid], excl = incl - h;
        if (rank >= excl && rank < incl) sel_digit = tid, sel_rank = rank - excl;  // exactly one lane: rank < the keys under the prefix
        __syncthreads();
        prefix |= (unsigned long long)sel_digit << shift;
        rank = sel_rank;
        __syncthreads();
    }
    if (tid == 0) median[j] = __longlong_as_double((long long)prefix);
}

// The centre of the camera (W, w): C_i = -((W[0][i]*w0 + W[1][i]*w1) + W[2][i]*w2).
__device__ __forceinline__ void chain_centre(const double (&W)[9], const double (&w)[3], double* C) {
#pragma unroll
    for (int i = 0; i < 3; ++i) C[i] = pose_canonical(-((W[i] * w[0] + W[3 + i] * w[1]) + W[6 + i] * w[2]));
}

// out = R W (step 4's product rule).
__device__ __forceinline__ void chain_compose(const double (&R)[9], const double (&W)[9], double (&out)[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * i + k] = (R[3 * i] * W[k] + R[3 * i + 1] * W[3 + k]) + R[3 * i + 2] * W[6 + k];
}

// grid = 1, one lane.  About 230 f64 and 120 other vector instructions per pair (W_j, the train camera, both centres, the
// canonical NaNs), issued by one wave one after the other, and scalar loads: the walk is bound by that issue rate, not by its
// loads (issuing the loads of pair j + 1 ahead of the arithmetic of pair j was tried: 69 ms against 70 - 74 ms at 65535 pairs).
__global__ __launch_bounds__(64) void k_chain_walk(const vslam_pose* __restrict__ poses, const unsigned int* __restrict__ usable,
                                                   const double* __restrict__ median, int n_pairs, unsigned int min_links,
                                                   vslam_chain* __restrict__ chain) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double W[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, w[3] = {0, 0, 0}, scale = 1.0;
    int segment = 0;
    bool prev_valid = false;
    for (int j = 0; j < n_pairs; ++j) {
        const bool valid = poses[j].best >= 0;
        const unsigned int nl = j >= 1 ? usable[j] : 0u;
        const double ratio = j >= 1 ? median[j] : 0.0;
        const bool linked = j >= 1 && prev_valid && valid && nl >= min_links;
        if (linked) {
            double R[9], t[3], nW[9], nw[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = poses[j - 1].R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = poses[j - 1].t[k];
            chain_compose(R, W, nW);
            chain_apply(R, w, scale, t, nw);
#pragma unroll
            for (int k = 0; k < 9; ++k) W[k] = nW[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) w[k] = nw[k];
            scale = scale * ratio;
        } else {
            segment = j, scale = 1.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) W[k] = k % 4 == 0 ? 1.0 : 0.0;
            w[0] = w[1] = w[2] = 0.0;
        }
        vslam_chain out;
#pragma unroll
        for (int k = 0; k < 9; ++k) out.W[k] = pose_canonical(W[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) out.w[k] = pose_canonical(w[k]);
        if (valid) {
            double R[9], t[3], Wt[9], wt[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = poses[j].R[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = poses[j].t[k];
            chain_centre(W, w, out.C);
            chain_compose(R, W, Wt);
            chain_apply(R, w, scale, t, wt);
            chain_centre(Wt, wt, out.Ct);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) out.C[k] = out.Ct[k] = 0.0;
        }
        out.scale = pose_canonical(scale);
        out.ratio = ratio;
        out.n_links = nl;
        out.segment = segment;
        out.linked = linked ? 1 : 0;
        out.valid = valid ? 1 : 0;
        chain[j] = out;
        prev_valid = valid;
    }
}

// grid = (record blocks of 256, n_pairs).  The pair's chain record is read through addresses that are the same in every lane.
__global__ __launch_bounds__(CHAIN_REC_WG) void k_chain_map(ChainIn in, const vslam_chain* __restrict__ chain, double* __restrict__ map) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(in.counts, j, in.mcap);
    const size_t i = g3_record(blockIdx.x, CHAIN_REC_WG, threadIdx.x);
    if (i >= m || !chain[j].valid) return;
    const size_t o = ((size_t)j * in.mcap + i) * 3;
    const double qnan = __longlong_as_double(CHAIN_QNAN);
    double M[3] = {qnan, qnan, qnan};
    unsigned int q, t;
    if (chain_live(in, j, i, q, t)) {
        const vslam_chain& cj = chain[j];
        const double s = cj.scale;
        const double c0 = s * in.points[o] - cj.w[0], c1 = s * in.points[o + 1] - cj.w[1], c2 = s * in.points[o + 2] - cj.w[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) M[k] = pose_canonical((cj.W[k] * c0 + cj.W[3 + k] * c1) + cj.W[6 + k] * c2);
    }
    map[o] = M[0], map[o + 1] = M[1], map[o + 2] = M[2];
}

}  // namespace vslam
