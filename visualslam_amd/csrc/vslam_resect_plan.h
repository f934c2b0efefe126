// The host arithmetic of vslam_resect_dev (include/vslam.h, "resection") that needs no HIP: the argument checks in the ABI's
// order, and the grids and scratch sizes, all from the capacities (the counts live on the device).  Stated once, here, so
// that a host program can run it under the sanitizers with extreme capacities (tests/resect_plan_driver.cpp).  The walk over
// the correspondences has the shape of vslam_epipolar_dev's - lane = hypothesis, tiles of EPI_TILE records dealt round robin
// to nsplit workgroups - so those grids are epipolar_plan's over the observation capacity.
#pragma once
#include "vslam_epipolar_plan.h"

namespace vslam {

constexpr unsigned int RES_MODEL_WG = 64;  // hypotheses per k_res_models workgroup: one wave, 144 f64 of LDS per lane

struct __attribute__((aligned(8))) ResYuv {  // what k_res_score stages of one correspondence
    double Y[3], u, v;
};

// The message of the first failed check, without the stage in front, in the order of vslam_chain_dev's (null, struct_size,
// n_pairs, the parameters, the inputs, the buffers); nullptr: the call is valid.
inline const char* resect_check_args(const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                                     const double* points, const uint64_t* front_bits, uint32_t point_cap, const vslam_match* obs_matches,
                                     const uint32_t* obs_counts, uint32_t obs_cap, const vslam_point* train_points, uint32_t train_cap, int n_pairs,
                                     const vslam_resect_params* prm, const vslam_resect_out* out) {
    if (!prm || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_resect_out)) return "out->struct_size is not sizeof(vslam_resect_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (prm->n_hypotheses < 1 || prm->n_hypotheses > 65535) return "1 .. 65535 hypotheses";
    if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    if (const char* why = check_intrinsics(prm->K, "an intrinsic is not finite")) return why;
    if (const char* why = twoview_check_inputs(poses && matches && match_counts && points && front_bits, match_cap, point_cap, point_cap)) return why;
    if (const char* why = twoview_check_inputs(obs_matches && obs_counts && train_points, obs_cap, train_cap, train_cap)) return why;
    const size_t np = (size_t)n_pairs, fwords = twoview_fwords(obs_cap);
    OUT_NEEDS(out, models, vslam_resect, np);
    // np * obs_cap < 2^48 and np * n_hypotheses < 2^32: no element count wraps, and the byte counts are compared by division
    OUT_FITS(out, inlier_bits, uint64_t, np * fwords);
    OUT_FITS(out, hypotheses, vslam_resect_hyp, np * prm->n_hypotheses);
    OUT_FITS(out, correspondences, vslam_resect_corr, np * obs_cap);
    OUT_FITS(out, links, int32_t, np * obs_cap);
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y and z
// <= 65535) and no size wraps: n_pairs < 2^16, n_hypotheses < 2^16, the capacities < 2^32, a record <= 104 bytes - below 2^56.
struct ResectPlan : EpipolarPlan {  // over obs_cap: fwords, rec_blocks (k_res_corr, k_res_gather, k_res_flags), model_blocks,
                                    // score_blocks, tiles, nsplit, hyp_elems, flag_words (the usable words; and the inlier words)
    unsigned int struct_rec_blocks;  // grid.x of k_chain_link over the structure side's match_cap
    unsigned int struct_fwords;      // ballot words per pair of front_bits
    unsigned int link_pairs;         // n_pairs - 1: grid.y of k_chain_link (0: not launched)
    size_t table_elems;              // scratch: the link table, uint32 [link_pairs][point_cap]
    size_t rec_elems;                // scratch: {b, a} per observation record, its dense list, and the dense correspondences: [n_pairs][obs_cap] each
    size_t pair_elems;               // scratch: n_corr, uint32 [n_pairs]
};

inline ResectPlan resect_plan(uint32_t match_cap, uint32_t point_cap, uint32_t obs_cap, int n_pairs, uint32_t n_hypotheses) {
    static_assert(RES_MODEL_WG == EPI_MODEL_WG, "model_blocks is epipolar_plan's");
    ResectPlan p{};
    static_cast<EpipolarPlan&>(p) = epipolar_plan(obs_cap, n_pairs, n_hypotheses);
    const TwoViewPlan st = twoview_plan(match_cap, n_pairs);
    p.struct_rec_blocks = st.rec_blocks, p.struct_fwords = st.fwords;
    const LinkTable lt = link_table(point_cap, n_pairs);
    p.link_pairs = lt.link_pairs, p.table_elems = lt.elems;
    p.rec_elems = (size_t)n_pairs * obs_cap;
    p.pair_elems = (size_t)n_pairs;
    return p;
}

}  // namespace vslam
