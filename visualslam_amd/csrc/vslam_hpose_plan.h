// The host arithmetic of vslam_hpose_dev (include/vslam.h, "pose from homography") that needs no HIP: the argument checks in
// the ABI's order, and the grids and scratch sizes, all from the capacities (the counts live on the device).  Stated once,
// here, so that a host program can run it under the sanitizers with extreme capacities (tests/hpose_plan_driver.cpp).
#pragma once
#include "vslam_pose_plan.h"

namespace vslam {

constexpr unsigned int HPOSE_PAIR_WG = 64;             // pairs (lanes) per k_hpose_candidates / k_hpose_select workgroup: one wave
constexpr unsigned int HPOSE_REC_WG = TWOVIEW_REC_WG;  // match records (lanes) per k_hpose_vote / k_hpose_points workgroup

// The message of the first failed check, without the stage in front, in the order of vslam_pose_dev's (null, struct_size,
// n_pairs, the parameters, the inputs, the buffers); nullptr: the call is valid.  priors is optional and is not looked at.
inline const char* hpose_check_args(const vslam_homography* models, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                                    const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap,
                                    int n_pairs, const vslam_hpose_params* prm, const vslam_hpose_out* out) {
    if (!prm || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_hpose_out)) return "out->struct_size is not sizeof(vslam_hpose_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (const char* why = check_intrinsics(prm->K)) return why;
    if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    if (!std::isfinite(prm->min_spread) || !(prm->min_spread > 0.0)) return "min_spread must be finite and positive";
    if (prm->ambiguous_den == 0) return "ambiguous_den must be positive";
    if (prm->only_degenerate != 0 && prm->only_degenerate != 1) return "only_degenerate must be 0 or 1";
    if (prm->reserved != 0) return "reserved must be 0";
    if (const char* why = twoview_check_inputs(models && matches && match_counts && query_points && train_points, match_cap, query_cap, train_cap)) return why;
    const size_t np = (size_t)n_pairs, fwords = twoview_fwords(match_cap);
    OUT_NEEDS(out, poses, vslam_pose, np);
    OUT_NEEDS(out, info, vslam_hpose, np);
    OUT_FITS(out, candidates, vslam_hpose_cand[4], np);
    // np * match_cap < 2^48: the element count cannot wrap, and the byte count is compared by division
    OUT_FITS(out, points, double[3], np * match_cap);
    OUT_FITS(out, front_bits, uint64_t, np * fwords);
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y <=
// 65535) and no size wraps: n_pairs < 2^16, the capacities < 2^32, a record <= 128 bytes.
struct HposePlan : TwoViewPlan {  // (rec_blocks: grid.x of k_hpose_vote and k_hpose_points, and of k_epi_coords)
    unsigned int pair_blocks;  // grid.x of k_hpose_candidates and k_hpose_select
    size_t cand_elems;         // scratch when the caller gives no candidates buffer
    size_t invd_elems;         // scratch: |T| of the two signs, f64 [n_pairs][2]
};

inline HposePlan hpose_plan(uint32_t match_cap, int n_pairs) {
    HposePlan p{};
    static_cast<TwoViewPlan&>(p) = twoview_plan(match_cap, n_pairs);
    const size_t np = (size_t)n_pairs;
    p.pair_blocks = (unsigned int)((np + HPOSE_PAIR_WG - 1) / HPOSE_PAIR_WG);
    p.cand_elems = np * 4;
    p.invd_elems = np * 2;
    return p;
}

}  // namespace vslam
