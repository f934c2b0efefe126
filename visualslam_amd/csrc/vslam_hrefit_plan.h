// The host arithmetic of vslam_hrefit_dev (include/vslam.h, "homography: least-squares refit over the inliers") that needs no
// HIP: the argument checks in the ABI's order, and the grids and scratch sizes, all from the capacities (the counts live on
// the device).  Stated once, here, so that a host program can run it under the sanitizers with extreme capacities
// (tests/hrefit_plan_driver.cpp).  The block of the ordered sum and the per-pair workgroup are the refit of F's
// (vslam_refit_plan.h): the two stages sum the same way.
#pragma once
#include "vslam_refit_plan.h"

namespace vslam {

constexpr unsigned int HREFIT_SUMS = 24;  // the widest pass: A_k, B_k, C_k, D_k for the six index pairs of a symmetric 3 x 3 block

// The per-pair record of the scratch: what the rounds carry from kernel to kernel.
struct HRefitState {
    vslam_homography in;      // models_in[j], read once (models may be the same buffer)
    double Hcur[9], Gcur[9];  // the model kept so far
    double Hcand[9], Gcand[9];  // the model whose members the next count pass counts: the input, then each round's (H_new, G_new)
    double cqx, cqy, ctx, cty, sq, st;  // step 2 of the round under way
    unsigned int n_cur, n_before, accepted;
    int stop;                 // REFIT_RUNNING until the pair stops
};

// The message of the first failed check, without the stage in front, in the order of refit_check_args (null, struct_size,
// n_pairs, the parameters, the inputs, the buffers); nullptr: the call is valid.
inline const char* hrefit_check_args(const vslam_homography* models_in, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                                     const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap,
                                     int n_pairs, const vslam_epipolar* epipolar_models, const vslam_hrefit_params* prm, const vslam_hrefit_out* out) {
    if (!prm || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_hrefit_out)) return "out->struct_size is not sizeof(vslam_hrefit_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (prm->rounds < 1 || prm->rounds > 8) return "1 .. 8 rounds";
    if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    if (epipolar_models && prm->degenerate_den == 0) return "degenerate_den must be positive";
    if (const char* why = twoview_check_inputs(models_in && matches && match_counts && query_points && train_points, match_cap, query_cap, train_cap)) return why;
    const size_t np = (size_t)n_pairs, fwords = twoview_fwords(match_cap);
    OUT_NEEDS(out, models, vslam_homography, np);
    OUT_FITS(out, info, vslam_hrefit, np);
    OUT_FITS(out, inlier_bits, uint64_t, np * fwords);
    if (out->inliers && (!out->inlier_counts || out->inlier_cap == 0)) return "inliers needs inlier_counts and an inlier_cap";
    OUT_FITS(out, inliers, vslam_match, np * out->inlier_cap);
    OUT_FITS(out, inlier_counts, uint32_t, np);
    if (out->gated_models && !epipolar_models) return "gated_models needs epipolar_models";
    OUT_FITS(out, gated_models, vslam_epipolar, np);
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y <=
// 65535) and no size wraps: n_pairs < 2^16, at most 2^20 blocks per pair, 24 f64 per block - below 2^44 bytes; a state record
// is 520 bytes.
struct HRefitPlan : TwoViewPlan {  // (rec_blocks: grid.x of k_epi_coords and k_hom_flags)
    unsigned int sum_blocks;   // grid.x of the streaming kernels: blocks of the ordered sum per pair, from the capacity
    unsigned int pair_blocks;  // grid.x of the per-pair kernels
    size_t partial_elems;      // scratch: [n_pairs][sum_blocks][HREFIT_SUMS] f64 block sums, reused by the three passes
    size_t state_elems;        // scratch: HRefitState [n_pairs]
    size_t flag_words;         // scratch when the list is asked for without inlier_bits
};

inline HRefitPlan hrefit_plan(uint32_t match_cap, int n_pairs) {
    HRefitPlan p{};
    static_cast<TwoViewPlan&>(p) = twoview_plan(match_cap, n_pairs);
    const size_t np = (size_t)n_pairs;
    p.sum_blocks = (unsigned int)(((size_t)match_cap + REFIT_BLOCK - 1) / REFIT_BLOCK);
    p.pair_blocks = (unsigned int)((np + REFIT_PAIR_WG - 1) / REFIT_PAIR_WG);
    p.partial_elems = np * p.sum_blocks * HREFIT_SUMS;
    p.state_elems = np;
    p.flag_words = np * p.fwords;
    return p;
}

}  // namespace vslam
