// Mutual (cross-check) matching (include/vslam.h, "mutual matching"): the matcher's nearest-two search of every query row, and in
// the same pass the REVERSE nearest of every train row - the query row of smallest d2, ties to the lowest query index.  d2 is
// symmetric bit for bit, so the reverse nearest is what the matcher would write with the sets swapped, and the distance tile
// that decides it is the one the forward search already holds.
//   k_match_nn2_mutual   : k_match_nn2's walk (kernels_match.hip.h) over the same shared steps (kernels_match_common.hip.h): tiling,
//                          split dealing, MFMA chain, forward update and MatchPart output.  In the epilogue a lane owns one train column of a 32 x 32 block and
//                          walks 16 query rows of it: the column minimum is taken in that walk, over the rows that are in use
//                          and defined (one ballot over the wave's 32 rows, a scalar mask), as (key, q) with key the ordered
//                          integer map of d2.  The two halves of a wave merge by one 64-bit shuffle, the four waves through LDS,
//                          and one wave issues one 64-lane atomicMin of (key << 32) | q per train tile: 512 contiguous bytes of
//                          rev [pair][train.cap].  A minimum over integers: no bit of rev depends on the order the workgroups
//                          arrive in.  With SAME_OCT the query tile's octaves live in LDS (the parent's 16 registers per lane
//                          and the column minimum do not fit together without scratch).
//   k_match_mutual_merge : match_merge_rows; the acceptance adds that rev[index] names this query row
//   k_match_rnn_write    : rev -> vslam_rnn for the train rows in use (the key mapped back to the bits of d2)
// rev is preset to all ones (nothing offered) before every launch.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/vslam.h"
#include "kernels_match_common.hip.h"

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

    float a[64];
    match_load_a(a, Q, p, min(qbase + wave * 32 + col, nq - 1), h);
    // the 16 query rows of this lane's accumulator registers.  Rows past nq are loaded as clamped copies of row nq - 1: the forward
    // search never publishes them, the reverse search must not hear of them, nor of a row whose `defined` byte is 0 - wmask below
    // says which rows take part in the column minimum.
    const unsigned int row0 = qbase + wave * 32 + 4 * h;  // query row of r: row0 + match_cd_row(r, 0), ascending in r
    float qn[16], best[16], second[16];
    int index[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        qn[r] = qnorm[(size_t)p * Q.cap + min(row0 + match_cd_row(r, 0), nq - 1)];
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

    const unsigned int ntiles = (nt + MT_T - 1) / MT_T;
    float4 pf[8];
    float pnb = 0.0f;
    int ptk = 0;
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

    const float4 *b0p = match_b_ptr(s_b, 0, col, h), *b1p = match_b_ptr(s_b, 1, col, h);
    unsigned int tile = split;
    bool pending = false;
    if (tile < ntiles) match_tile_gload<SAME_OCT>(pf, pnb, ptk, T, tnorm, p, nt, tile, t);
    while (tile < ntiles) {
        __syncthreads();  // the previous tile has been read, and its column minima are in s_rev
        if (pending) publish(tile - nsplit);
        match_tile_lstore(pf, pnb, ptk, s_b, s_nb, s_tk, t);
        __syncthreads();
        const unsigned int next = tile + nsplit;
        if (next < ntiles) match_tile_gload<SAME_OCT>(pf, pnb, ptk, T, tnorm, p, nt, next, t);  // in flight under the MFMAs
        f32x16 acc0, acc1;
        match_mfma_chain(a, b0p, b1p, acc0, acc1);
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
                match_nn2_update(best, second, index, r, d2, j);
                const bool clt = d2 < cbest && (h ? (wmask >> match_cd_row(r, 1)) & 1 : (wmask >> match_cd_row(r, 0)) & 1);
                crow = clt ? match_cd_row(r, 0) : crow;
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

    match_finish(best, second, index, s_res, part, Q, p, nsplit, split, qbase, nq, t, wave, col, h);
}

// grid = (ceil(Q.cap / MT_ROW_WG), pairs).  rev is complete: the launch follows k_match_nn2_mutual on the same stream.
__global__ __launch_bounds__(256) void k_match_mutual_merge(const vslam_desc_sets Q, const MatchPart* __restrict__ part, int nsplit, float ratio2,
                                                             const unsigned long long* __restrict__ rev, unsigned int tcap,
                                                             vslam_nn2* __restrict__ nn, unsigned long long* __restrict__ flags, unsigned int fwords) {
    match_merge_rows(Q, part, nsplit, ratio2, nn, flags, fwords,
                     [=](int p, unsigned int q, float, int i) { return (unsigned int)rev[(size_t)p * tcap + (unsigned int)i] == q; });  // (i < the train count <= tcap)
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
