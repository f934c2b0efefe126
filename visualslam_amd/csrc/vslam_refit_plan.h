// The host arithmetic of vslam_refit_dev (include/vslam.h, "fundamental matrix: least-squares refit over the inliers") that
// needs no HIP: the argument checks in the ABI's order, and the grids and scratch sizes, all from the capacities (the counts
// live on the device).  Stated once, here, so that a host program can run it under the sanitizers with extreme capacities
// (tests/refit_plan_driver.cpp).
#pragma once
#include "vslam_epipolar_plan.h"

namespace vslam {

constexpr unsigned int REFIT_WG = 256;        // lanes of a streaming workgroup: the 256 slots of the header's ordered sum
constexpr unsigned int REFIT_PER_LANE = 16;   // records a slot adds before the tree
constexpr unsigned int REFIT_BLOCK = REFIT_WG * REFIT_PER_LANE;  // 4096: the records of one block of the ordered sum
constexpr unsigned int REFIT_SUMS = 45;       // the widest pass: the upper triangle of the 9 x 9 moment matrix
constexpr unsigned int REFIT_PAIR_WG = 64;    // pairs (lanes) per workgroup of the per-pair kernels: one wave
constexpr int REFIT_RUNNING = -1;             // RefitState::stop of a pair that has not stopped
static_assert(REFIT_BLOCK == 4096, "the block of the ordered sum is part of the ABI");

// The per-pair record of a refit's scratch: what the rounds carry from kernel to kernel, and what the shared steps
// (kernels_estimate.hip.h) need to know of the stage - Rec its model record, Model_ the blocks of it that are refitted, Info_
// its info record, the fewest members a round works from, and the f64 per block of its partial sums (its widest pass).
template <class Rec, class Model_, class Info_, unsigned int MIN_MEMBERS_, unsigned int SUMS_>
struct RefitRounds {
    using Model = Model_;
    using Info = Info_;
    static constexpr unsigned int MIN_MEMBERS = MIN_MEMBERS_, SUMS = SUMS_;
    Rec in;       // models_in[j], read once (models may be the same buffer)
    Model cur;    // the model kept so far
    Model cand;   // the model whose members the next count pass counts: the input, then each round's new model
    double cqx, cqy, ctx, cty, sq, st;  // step 2 of the round under way
    unsigned int n_cur, n_before, accepted;
    int stop;     // REFIT_RUNNING until the pair stops
};
struct RefitState : RefitRounds<vslam_epipolar, EpiModel, vslam_refit, 8, REFIT_SUMS> {};  // (a type of its own: the kernels' symbols name it)

// The message of the first failed check, without the stage in front, in the order of vslam_epipolar_dev's (null, struct_size,
// n_pairs, the parameters, the inputs, the buffers); nullptr: the call is valid.
inline const char* refit_check_args(const vslam_epipolar* models_in, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                                    const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap,
                                    int n_pairs, const vslam_refit_params* prm, const vslam_refit_out* out) {
    if (!prm || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_refit_out)) return "out->struct_size is not sizeof(vslam_refit_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (prm->rounds < 1 || prm->rounds > 8) return "1 .. 8 rounds";
    if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    if (const char* why = twoview_check_inputs(models_in && matches && match_counts && query_points && train_points, match_cap, query_cap, train_cap)) return why;
    const size_t np = (size_t)n_pairs, fwords = twoview_fwords(match_cap);
    OUT_NEEDS(out, models, vslam_epipolar, np);
    OUT_FITS(out, info, vslam_refit, np);
    return twoview_check_lists(out, np, fwords);
}

// Grids and scratch of one valid call of either refit with n_pairs >= 1, `sums` the f64 per block of the stage.  Every grid
// dimension stays within HIP's limits (x < 2^31, y <= 65535) and no size wraps: n_pairs < 2^16, at most 2^20 blocks per pair,
// at most 45 f64 per block - below 2^45 bytes.
struct RefitPlan : TwoViewPlan {  // (rec_blocks: grid.x of k_epi_coords and of the flags kernel)
    unsigned int sum_blocks;   // grid.x of the streaming kernels: blocks of the ordered sum per pair, from the capacity
    unsigned int pair_blocks;  // grid.x of the per-pair kernels
    size_t partial_elems;      // scratch: [n_pairs][sum_blocks][sums] f64 block sums, reused by the three passes
    size_t state_elems;        // scratch: the stage's state record, [n_pairs]
    size_t flag_words;         // scratch when the list is asked for without inlier_bits
};

inline RefitPlan refit_plan(uint32_t match_cap, int n_pairs, unsigned int sums = REFIT_SUMS) {
    RefitPlan p{};
    static_cast<TwoViewPlan&>(p) = twoview_plan(match_cap, n_pairs);
    const size_t np = (size_t)n_pairs;
    p.sum_blocks = (unsigned int)(((size_t)match_cap + REFIT_BLOCK - 1) / REFIT_BLOCK);
    p.pair_blocks = (unsigned int)((np + REFIT_PAIR_WG - 1) / REFIT_PAIR_WG);
    p.partial_elems = np * p.sum_blocks * sums;
    p.state_elems = np;
    p.flag_words = np * p.fwords;
    return p;
}

}  // namespace vslam
