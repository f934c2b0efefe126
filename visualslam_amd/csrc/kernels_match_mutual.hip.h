// Mutual (cross-check) matching (include/vslam.h, "mutual matching"): the matcher's nearest-two search of every query row, and in
// the same pass the REVERSE nearest of every train row - the query row of smallest d2, ties to the lowest query index.  d2 is
// symmetric bit for bit, so the reverse nearest is what the matcher would write with the sets swapped, and the distance tile
// that decides it is the one the forward search already holds.
//   k_match_nn2_mutual   : a sibling of k_match_nn2 (kernels_match.hip.h): the same tiling, split dealing, MFMA chain, forward
//                          update and MatchPart output.  In the epilogue a lane owns one train column of a 32 x 32 block and
//                          walks 16 query rows of it: the column minimum is taken in that walk, over the rows that are in use
//                          and defined (one ballot over the wave's 32 rows, a scalar mask), as (key, q) with key the ordered
//                          integer map of d2.  The two halves of a wave merge by one 64-bit shuffle, the four waves through LDS,
//                          and one wave issues one 64-lane atomicMin of (key << 32) | q per train tile: 512 contiguous bytes of
//                          rev [pair][train.cap].  A minimum over integers: no bit of rev depends on the order the workgroups
//                          arrive in.  With SAME_OCT the query tile's octaves live in LDS (the parent's 16 registers per lane
//                          and the column minimum do not fit together without scratch).
//   k_match_mutual_merge : k_match_merge's fold and ratio test; the flag is accept && rev[index] names this query row
//   k_match_rnn_write    : rev -> vslam_rnn for the train rows in use (the key mapped back to the bits of d2)
// rev is preset to all ones (nothing offered) before every launch.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_match_common.hip.h"  // MT_Q, MT_T, MT_LD, MT_MAX_SPLIT, MatchPart, match_merge

namespace vslam {

constexpr unsigned long long REV_NONE = ~0ull;  // above every (key, q) of a d2 < +inf: such a key is below 0xff800000

// The ordered map of f32: a < b as floats iff key(a) < key(b) as unsigned, for everything but NaN.  + 0.0f folds -0 into +0.
__device__ __forceinline__ unsigned int rev_key(float d2) {
    const unsigned int u = __float_as_uint(d2 + 0.0f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float rev_unkey(unsigned int key) {
    return __uint_as_float((key >> 31) ? key ^ 0x80000000u : ~key);
}

// grid = (ceil(Q.cap / MT_Q), nsplit, pairs).  part: [pair][split][Q.cap]; rev: [pair][T.cap], preset to REV_NONE.
template <bool SAME_OCT>
__global__ __launch_bounds__(256, 2) void k_match_nn2_mutual(const vslam_desc_sets Q, const vslam_desc_sets T, const float* __restrict__ qnorm,
                                                           const float* __restrict__ tnorm, int nsplit, MatchPart* __restrict__ part,
                                                           unsigned long long* __restrict__ rev) {
    __shared__ float4 s_b[MT_T * MT_LD / 4];
    __shared__ float s_nb[MT_T];
    __shared__ int s_tk[MT_T];
    __shared__ MatchPart s_res[MT_Q];
    __shared__ unsigned long long s_rev[4][MT_T];
    __shared__ int4 s_qk[SAME_OCT ? MT_Q / 4 : 1];  // the query tile's octaves: 16 more registers per lane would not fit
    const int p = blockIdx.z, split = blockIdx.y, t = threadIdx.x, lane = t & 63, col = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);  // stated as uniform: what is indexed by it is addressed from scalar registers
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
    // the 16 query rows of this lane's accumulator registers (the C / D map of the 32 x 32 forms).  Rows past nq are loaded as
    // clamped copies of row nq - 1: the forward search never publishes them, the reverse search must not hear of them, nor of a
    // row whose `defined` byte is 0 - wmask below says which rows take part in the column minimum.
    const unsigned int row0 = qbase + wave * 32 + 4 * h;  // query row of r: row0 + (r & 3) + 8 * (r >> 2), ascending in r
    float qn[16], best[16], second[16];
    int index[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const unsigned int own = row0 + (r & 3) + 8 * (r >> 2);
        const unsigned int qrow = min(own, nq - 1);
        qn[r] = qnorm[(size_t)p * Q.cap + qrow];
        best[r] = second[r] = inf;
        index[r] = -1;
    }
    if (SAME_OCT && t < MT_Q)  // (read after the loop's barriers)
        reinterpret_cast<int*>(s_qk)[t] = Q.points[(size_t)p * Q.cap + min(qbase + t, nq - 1)].octave;
    unsigned int wmask;  // bit i: row i of the wave's 32 takes part; the same in every lane
    {
        const unsigned int own = qbase + wave * 32 + col;
        wmask = (unsigned int)__ballot(own < nq && (!Q.defined || Q.defined[(size_t)p * Q.cap + own]));
    }

    // one train tile: 64 rows x 16 groups of eight floats, four groups per thread; norm and octave of row t by thread t < 64
    const unsigned int ntiles = (nt + MT_T - 1) / MT_T;
    float4 pf[8];
    float pnb = 0.0f;
    int ptk = 0;
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
            pnb = alive ? tnorm[(size_t)p * T.cap + j] : __int_as_float(0x7fc00000);  // NaN: a skipped row never wins, either way
            ptk = SAME_OCT && j < nt ? T.points[(size_t)p * T.cap + j].octave : 0;
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
    };
    // the four waves' column minima of train tile `done` lie in s_rev (written before the barrier the caller has just passed, not
    // written again before the next one): wave 0 folds them and offers train row done * MT_T + lane its winner
    auto publish = [&](unsigned int done) {
        if (wave == 0) {
            unsigned long long v = s_rev[0][lane];
#pragma unroll
            for (int w = 1; w < 4; ++w) {
                const unsigned long long o = s_rev[w][lane];
                v = o < v ? o : v;
            }
            const unsigned int j = done * MT_T + lane;
            if (j < nt && v != REV_NONE) atomicMin(rev + (size_t)p * T.cap + j, v);
        }
    };

    const float4* b0p = s_b + (col * MT_LD) / 4 + h;
    const float4* b1p = s_b + ((32 + col) * MT_LD) / 4 + h;
    unsigned int tile = split;
    bool pending = false;
    if (tile < ntiles) gload(tile);
    while (tile < ntiles) {
        __syncthreads();  // the previous tile has been read, and its column minima are in s_rev
        if (pending) publish(tile - nsplit);
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
        // epilogue: this lane's train column of each block against its 16 query rows, ascending train index for the forward
        // update, ascending query row for the column minimum (a strict < keeps the lowest row of a tie; NaN and +inf never pass)
        auto select = [&](const f32x16& acc, int blk) -> unsigned long long {
            const float nb = s_nb[32 * blk + col];
            const int tk = s_tk[32 * blk + col];
            const int j = (int)(tile * MT_T) + 32 * blk + col;
            float cbest = inf;
            int crow = 0;
            int4 qk4 = make_int4(0, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float s = acc[r];
                float d2 = (qn[r] + nb) - 2.0f * s;
                if (SAME_OCT) {  // rows 8 g + 4 h .. + 3 of the wave's 32: one broadcast read per four rows
                    if ((r & 3) == 0) qk4 = s_qk[wave * 8 + 2 * (r >> 2) + h];
                    const int qk = (r & 3) == 0 ? qk4.x : (r & 3) == 1 ? qk4.y : (r & 3) == 2 ? qk4.z : qk4.w;
                    if (qk != tk) d2 = inf;
                }
                const bool lt = d2 < best[r];
                const float s2 = d2 < second[r] ? d2 : second[r];
                second[r] = lt ? best[r] : s2;
                index[r] = lt ? j : index[r];
                best[r] = lt ? d2 : best[r];
                const bool clt = d2 < cbest && (h ? (wmask >> ((r & 3) + 8 * (r >> 2) + 4)) & 1 : (wmask >> ((r & 3) + 8 * (r >> 2))) & 1);
                crow = clt ? (r & 3) + 8 * (r >> 2) : crow;
                cbest = clt ? d2 : cbest;
            }
            return cbest < inf ? ((unsigned long long)rev_key(cbest) << 32) | (row0 + crow) : REV_NONE;
        };
        // the other half of the wave holds the same column over the other 16 rows: half `blk` stores the merged pair, so that
        // s_rev[wave][l] is the minimum of train row tile * MT_T + l over the wave's 32 query rows
        auto column = [&](const f32x16& acc, int blk) {
            const unsigned long long mine = select(acc, blk);
            const unsigned long long got = __shfl_xor(mine, 32);
            if (h == blk) s_rev[wave][lane] = got < mine ? got : mine;
        };
        column(acc0, 0);
        column(acc1, 1);
        pending = true;
        tile = next;
    }
    __syncthreads();
    if (pending) publish(tile - nsplit);

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

// grid = (ceil(Q.cap / 256), pairs); flags: [pair][fwords], fwords = ceil(Q.cap / 64).  rev is complete: the launch follows
// k_match_nn2_mutual on the same stream.
__global__ __launch_bounds__(256) void k_match_mutual_merge(const vslam_desc_sets Q, const MatchPart* __restrict__ part, int nsplit, float ratio2,
                                                             const unsigned long long* __restrict__ rev, unsigned int tcap,
                                                             vslam_nn2* __restrict__ nn, unsigned long long* __restrict__ flags, unsigned int fwords) {
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
        accept = i >= 0 && (s == inf || b < __fmul_rn(ratio2, s));
        accept = accept && (unsigned int)rev[(size_t)p * tcap + (unsigned int)i] == q;  // (i < the train count <= tcap)
    }
    const unsigned long long w = __ballot(accept);
    if ((threadIdx.x & 63) == 0 && q / 64 < fwords) flags[(size_t)p * fwords + q / 64] = w;
}

// grid = (ceil(T.cap / 256), pairs).  Rows past the train count are left untouched.
__global__ __launch_bounds__(256) void k_match_rnn_write(const vslam_desc_sets T, const unsigned long long* __restrict__ rev,
                                                          vslam_rnn* __restrict__ rnn) {
    const int p = blockIdx.y;
    const unsigned int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= min(T.counts[p], T.cap)) return;
    const unsigned long long v = rev[(size_t)p * T.cap + j];
    vslam_rnn r;
    r.index = v == REV_NONE ? -1 : (int)(unsigned int)v;
    r.dist2 = v == REV_NONE ? match_inf() : rev_unkey((unsigned int)(v >> 32));
    rnn[(size_t)p * T.cap + j] = r;
}

}  // namespace vslam
