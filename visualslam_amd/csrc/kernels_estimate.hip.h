// The steps that the model-estimation stages share, each stated once.  A stage's __global__ kernels (kernels_epipolar.hip.h,
// kernels_homography.hip.h, kernels_resect.hip.h, kernels_sim3.hip.h; kernels_refit.hip.h, kernels_hrefit.hip.h) are a few lines over these
// bodies: every body is inlined, and a kernel's name, signature and device code are what they were when it was written out
// (profiles/estimators_isa_identity.txt).
//   RANSAC       : ransac_select (the winner of a pair), ransac_flags (its ballot words)
//   refit rounds : refit_pass (a streaming pass: the idle test, the model, one block of the ordered sum) with the add steps of
//                  the count and distance passes, and the per-pair steps refit_init, refit_begin, refit_scale
// A stage is named by its model: the 3 x 3 blocks a lane keeps in registers (EpiModel, HomModel: vslam_epipolar_plan.h;
// ResModel, Sim3Model: here).  model_copy<Model> copies them between any two things that name the blocks as the ABI does - a model, a
// hypothesis, a pair's record -, and the stages over EpiXY records have model_inlier.  What stays with its stage: the *_models
// kernels (k_epi_models stands at its register budget, kernels_geom3.hip.h), the *_score kernels (behind an inlined body their
// scalar prologue is scheduled otherwise), k_res_flags (it recomputes the correspondence), k_hom_verdict, the add step of the
// moments passes and steps 3 - 5 of the solve kernels.
// The bodies' pointer parameters carry no __restrict__ of their own, on purpose: the kernels' parameters do, and a second
// qualifier on an inlined body gives the compiler other alias scopes - and the kernel another schedule.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/vslam.h"
#include "kernels_geom3.hip.h"
#include "vslam_refit_plan.h"

namespace vslam {

struct ResModel {  // the pose of a resection hypothesis or pair
    double R[9], t[3];
};
struct Sim3Model {  // the similarity of a loop alignment hypothesis or slot
    double s, R[9], t[3];
};
// d's blocks = s's: the blocks are Model's, d and s anything that names them so.
template <class Model, class D, class S>
__device__ __forceinline__ void model_copy(D& d, const S& s) {
    if constexpr (std::is_same<Model, EpiModel>::value) {
#pragma unroll
        for (int i = 0; i < 9; ++i) d.F[i] = s.F[i];
    } else if constexpr (std::is_same<Model, HomModel>::value) {
#pragma unroll
        for (int i = 0; i < 9; ++i) d.H[i] = s.H[i], d.G[i] = s.G[i];
    } else {
        static_assert(std::is_same<Model, ResModel>::value || std::is_same<Model, Sim3Model>::value, "EpiModel, HomModel, ResModel or Sim3Model");
#pragma unroll
        for (int i = 0; i < 9; ++i) d.R[i] = s.R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) d.t[i] = s.t[i];
        if constexpr (std::is_same<Model, Sim3Model>::value) d.s = s.s;
    }
}
// A record whose every block reads 0.0: the "no model" of the ABI.
struct ZeroBlocks {
    struct Block {
        __device__ double operator[](int) const { return 0.0; }
    } F, H, G, R, t;
    static constexpr double s = 0.0;  // (the scale of a Sim3Model; not a member of the record: the layout stays)
};
__device__ __forceinline__ bool model_inlier(const EpiModel& m, const EpiXY& p, double max_dist2) { return epi_inlier(m.F, p, max_dist2); }
__device__ __forceinline__ bool model_inlier(const HomModel& m, const EpiXY& p, double max_dist2) { return hom_inlier(m.H, m.G, p, max_dist2); }

// ---- RANSAC ----

// One workgroup of 256 per pair, hy its NH hypotheses, *dst its record.  key = valid ? (inliers + 1) << 16 | (65535 - h) : 0:
// the maximum is the most inliers, then the lowest h (h < 65536; inliers + 1 < 2^33 needs 64 bits).  Thread 0 writes the
// record: header(out) sets the fields that are the stage's own, the rest is stated here - n_valid, and the winner's model,
// n_inliers and best; all zero and best = -1 without a valid hypothesis.
template <class Model, class Hyp, class Rec, class Header>
__device__ __forceinline__ void ransac_select(const Hyp* hy, unsigned int NH, Rec* dst, Header header) {
    __shared__ unsigned long long skey[4];
    __shared__ unsigned int sval[4];
    unsigned long long key = 0;
    unsigned int nvalid = 0;
    for (unsigned int h = threadIdx.x; h < NH; h += 256)
        if (hy[h].valid) {
            ++nvalid;
            const unsigned long long k = ((unsigned long long)hy[h].inliers + 1ull) << 16 | (unsigned long long)(65535u - h);
            key = max(key, k);
        }
    for (int off = 32; off >= 1; off >>= 1) {
        key = max(key, (unsigned long long)__shfl_down(key, off));
        nvalid += __shfl_down(nvalid, off);
    }
    if ((threadIdx.x & 63) == 0) skey[threadIdx.x >> 6] = key, sval[threadIdx.x >> 6] = nvalid;
    __syncthreads();
    if (threadIdx.x == 0) {
        key = max(max(skey[0], skey[1]), max(skey[2], skey[3]));
        Rec out;
        header(out);
        out.n_valid = sval[0] + sval[1] + sval[2] + sval[3];
        if (key) {
            const unsigned int best = 65535u - (unsigned int)(key & 0xffffull);
            model_copy<Model>(out, hy[best]);
            out.n_inliers = hy[best].inliers;
            out.best = (int)best;
        } else {
            model_copy<Model>(out, ZeroBlocks{});
            out.n_inliers = 0;
            out.best = -1;
        }
        *dst = out;
    }
}

// grid = (record blocks, pairs): bit i % 64 of word i / 64 = record i is an inlier of the pair's model; the words that hold a
// record below the count are written (all zero without a winner: the model is zero), the others left alone.
template <class Model, class Rec>
__device__ __forceinline__ void ransac_flags(const EpiXY* xy, const unsigned int* counts, unsigned int mcap,
                                             const Rec* models, double max_dist2, unsigned long long* flags,
                                             unsigned int fwords) {
    const int j = blockIdx.y;
    const unsigned int m = g3_count(counts, j, mcap);
    const size_t i = g3_record(blockIdx.x, 256, threadIdx.x);
    if (!g3_wave_has_record(i, m)) return;
    Model M;
    model_copy<Model>(M, models[j]);
    bool in = false;
    if (i < m) in = model_inlier(M, xy[(size_t)j * mcap + i], max_dist2);
    const unsigned long long w = __ballot(in);
    g3_store_word(flags, j, fwords, i, g3_first_lane(threadIdx.x), w);
}

// ---- refit rounds ----
// State is the stage's per-pair scratch record (RefitRounds, vslam_refit_plan.h): its model type, its minimum member count and
// the stride of its block sums come with it.

struct RefitNorm {  // step 2 of the round under way, as a streaming pass reads it
    double cqx, cqy, ctx, cty, sq, st;
};

// true: this workgroup has nothing to do - its pair has stopped, or its block lies past the pair's count.
template <class State>
__device__ __forceinline__ bool refit_idle(const State* __restrict__ state, const unsigned int* __restrict__ counts, unsigned int mcap) {
    return state[blockIdx.y].stop != REFIT_RUNNING || (size_t)blockIdx.x * REFIT_BLOCK >= g3_count(counts, blockIdx.y, mcap);
}

// One streaming pass, grid = (blocks of 4096 records, pairs): N sums over the members under the pair's candidate or kept
// model.  Add is made from the pair's RefitNorm and adds one member's terms: add(s, p).  A workgroup with nothing to do leaves
// before its first barrier (workgroup-uniform).
template <int N, bool CANDIDATE, class Add, class State>
__device__ __forceinline__ void refit_pass(const EpiXY* xy, const unsigned int* counts, unsigned int mcap, const State* state, double max_dist2,
                                           double* partial, unsigned int sum_blocks) {
    __shared__ double lds[N * 128];
    if (refit_idle(state, counts, mcap)) return;
    const State* st = state + blockIdx.y;
    typename State::Model M;
    model_copy<typename State::Model>(M, CANDIDATE ? st->cand : st->cur);
    const Add add{RefitNorm{st->cqx, st->cqy, st->ctx, st->cty, st->sq, st->st}};
    const auto member = [&](const EpiXY& p) { return model_inlier(M, p, max_dist2); };
    refit_block_sums<N, (int)State::SUMS>(xy, counts, mcap, partial, sum_blocks, lds, member, add);
}

// SUM(x), SUM(y), SUM(x'), SUM(y') and SUM(1.0) - the member count, exact in f64 - under the CANDIDATE model.
struct RefitCountAdd {
    RefitNorm nm;
    __device__ void operator()(double (&s)[5], const EpiXY& p) const {
        s[0] = s[0] + p.x, s[1] = s[1] + p.y, s[2] = s[2] + p.u, s[3] = s[3] + p.v, s[4] = s[4] + 1.0;
    }
};
// SUM(sqrt(dx*dx + dy*dy)) per side under the kept model.
struct RefitDistAdd {
    RefitNorm nm;
    __device__ void operator()(double (&s)[2], const EpiXY& p) const {
        const double dx = p.x - nm.cqx, dy = p.y - nm.cqy, du = p.u - nm.ctx, dv = p.v - nm.cty;
        s[0] = s[0] + sqrt(dx * dx + dy * dy);
        s[1] = s[1] + sqrt(du * du + dv * dv);
    }
};

// The per-pair steps: grid = (pair blocks of 64), one lane per pair.
// models_in -> the state.
template <class State, class Rec>
__device__ __forceinline__ void refit_init(const Rec* models_in, int n_pairs, State* state) {
    const int j = blockIdx.x * REFIT_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    State s;
    s.in = models_in[j];
    model_copy<typename State::Model>(s.cur, s.in);
    model_copy<typename State::Model>(s.cand, s.in);
    s.cqx = s.cqy = s.ctx = s.cty = s.sq = s.st = 0.0;
    s.n_cur = s.n_before = s.accepted = 0;
    s.stop = s.in.best < 0 ? 5 : REFIT_RUNNING;
    state[j] = s;
}

// Round r's first steps: the count pass before it belongs to round r - 1's new model (r >= 1: step 6, accept or stop 4) or to
// the input (r == 0: n_before); then step 1 and the centroids of step 2.  The launch with r == rounds closes the last round
// and writes models and info.  `models` may be the buffer refit_init read: it is written by that last launch only, so it is not
// __restrict__.
template <class State, class Rec>
__device__ __forceinline__ void refit_begin(const double* partial, unsigned int sum_blocks, const unsigned int* counts,
                                            unsigned int mcap, int n_pairs, unsigned int r, unsigned int rounds, State* state, Rec* models,
                                            typename State::Info* info) {
    const int j = blockIdx.x * REFIT_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    State* st = state + j;
    if (st->stop == REFIT_RUNNING) {
        double s[5];
        refit_pair_sums<5, (int)State::SUMS>(partial, j, sum_blocks, g3_count(counts, j, mcap), s);
        const unsigned int n = (unsigned int)s[4];
        bool running = true;
        if (r == 0) {
            st->n_before = st->n_cur = n;
        } else if (n >= st->n_cur) {  // step 6
            model_copy<typename State::Model>(st->cur, st->cand);
            st->n_cur = n;
            st->accepted += 1;
        } else {
            st->stop = 4;
            running = false;
        }
        if (running) {
            if (r == rounds) {
                st->stop = 0;
            } else if (st->n_cur < State::MIN_MEMBERS) {  // step 1
                st->stop = 1;
            } else {  // step 2, the centroids
                const double nd = (double)st->n_cur;
                st->cqx = s[0] / nd, st->cqy = s[1] / nd, st->ctx = s[2] / nd, st->cty = s[3] / nd;
            }
        }
    }
    if (r == rounds) {
        Rec out = st->in;
        if (st->stop != 5) {
            const typename State::Model& kept = st->cur;  // (written out: through model_copy k_refit_begin's registers are allocated otherwise)
            if constexpr (std::is_same<typename State::Model, EpiModel>::value) {
#pragma unroll
                for (int k = 0; k < 9; ++k) out.F[k] = kept.F[k];
            } else {
#pragma unroll
                for (int k = 0; k < 9; ++k) out.H[k] = kept.H[k], out.G[k] = kept.G[k];
            }
            out.n_inliers = st->n_cur;
        }
        models[j] = out;
        if (info) info[j] = typename State::Info{st->n_before, st->n_cur, st->accepted, st->stop};
    }
}

// The rest of step 2.
template <class State>
__device__ __forceinline__ void refit_scale(const double* partial, unsigned int sum_blocks, const unsigned int* counts,
                                            unsigned int mcap, int n_pairs, State* state) {
    const int j = blockIdx.x * REFIT_PAIR_WG + threadIdx.x;
    if (j >= n_pairs) return;
    State* st = state + j;
    if (st->stop != REFIT_RUNNING) return;
    double s[2];
    refit_pair_sums<2, (int)State::SUMS>(partial, j, sum_blocks, g3_count(counts, j, mcap), s);
    if (!refit_scales(s, st->n_cur, st->sq, st->st)) st->stop = 2;
}

}  // namespace vslam
