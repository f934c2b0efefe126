// The host arithmetic of vslam_homography_dev (include/vslam.h, "homography and the degeneracy verdict") that needs no HIP:
// the argument checks in the ABI's order, and the grids and scratch sizes, all from the capacities (the counts live on the
// device).  Stated once, here, so that a host program can run it under the sanitizers with extreme capacities
// (tests/homography_plan_driver.cpp).  The record walk has the shape of vslam_epipolar_dev's - lane = hypothesis, tiles of
// EPI_TILE records dealt round robin to nsplit workgroups - so the grids are epipolar_plan's.
#pragma once
#include "vslam_epipolar_plan.h"

namespace vslam {

constexpr unsigned int HOM_MODEL_WG = 64;  // hypotheses per k_hom_models workgroup: one wave, 72 f64 of LDS per lane
constexpr unsigned int HOM_PAIR_WG = 64;   // pairs (lanes) per k_hom_verdict workgroup

// The message of the first failed check, without the stage in front, in the order of vslam_epipolar_dev's (null, struct_size,
// n_pairs, the parameters, the inputs, the buffers); nullptr: the call is valid.
inline const char* homography_check_args(const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                                         const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap,
                                         int n_pairs, const vslam_epipolar* epipolar_models, const vslam_homography_params* prm,
                                         const vslam_homography_out* out) {
    if (!prm || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_homography_out)) return "out->struct_size is not sizeof(vslam_homography_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (prm->n_hypotheses < 1 || prm->n_hypotheses > 65535) return "1 .. 65535 hypotheses";
    if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    if (prm->degenerate_den == 0) return "degenerate_den must be positive";
    if (const char* why = twoview_check_inputs(matches && match_counts && query_points && train_points, match_cap, query_cap, train_cap)) return why;
    const size_t np = (size_t)n_pairs, fwords = twoview_fwords(match_cap);
    OUT_NEEDS(out, models, vslam_homography, np);
    if (const char* why = twoview_check_lists(out, np, fwords)) return why;
    OUT_FITS(out, hypotheses, vslam_homography_hyp, np * prm->n_hypotheses);
    if (out->gated_models && !epipolar_models) return "gated_models needs epipolar_models";
    OUT_FITS(out, gated_models, vslam_epipolar, np);
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y and z
// <= 65535) and no size wraps: n_pairs < 2^16, n_hypotheses < 2^16, the capacities < 2^32, a record <= 152 bytes - below 2^56.
struct HomographyPlan : EpipolarPlan {  // (model_blocks, score_blocks, tiles, nsplit, hyp_elems, flag_words: as named there)
    unsigned int pair_blocks;           // grid.x of k_hom_verdict
};

inline unsigned int hom_pair_blocks(int n_pairs) { return (unsigned int)(((size_t)n_pairs + HOM_PAIR_WG - 1) / HOM_PAIR_WG); }
inline HomographyPlan homography_plan(uint32_t match_cap, int n_pairs, uint32_t n_hypotheses) {
    static_assert(HOM_MODEL_WG == EPI_MODEL_WG, "model_blocks is epipolar_plan's");
    HomographyPlan p{};
    static_cast<EpipolarPlan&>(p) = epipolar_plan(match_cap, n_pairs, n_hypotheses);
    p.pair_blocks = hom_pair_blocks(n_pairs);
    return p;
}

}  // namespace vslam
