// The host arithmetic of vslam_chain_dev (include/vslam.h, "trajectory") that needs no HIP: the argument checks in the ABI's
// order, and the grids and scratch sizes, all from the capacities (the counts live on the device).  Stated once, here, so
// that a host program can run it under the sanitizers with extreme capacities (tests/chain_plan_driver.cpp).
#pragma once
#include "vslam_epipolar_plan.h"

namespace vslam {

constexpr unsigned int CHAIN_REC_WG = TWOVIEW_REC_WG;  // match records (lanes) per k_chain_link / k_chain_ratio / k_chain_map workgroup
constexpr unsigned int CHAIN_MEDIAN_WG = 256;          // lanes of the one k_chain_median workgroup of a pair: one per radix bin

// The message of the first failed check, without the stage in front, in the order of vslam_pose_dev's (null, struct_size,
// n_pairs, the parameters, the inputs, the buffers); nullptr: the call is valid.
inline const char* chain_check_args(const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                                    const double* points, const uint64_t* front_bits, uint32_t point_cap, int n_pairs,
                                    const vslam_chain_params* prm, const vslam_chain_out* out) {
    if (!prm || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_chain_out)) return "out->struct_size is not sizeof(vslam_chain_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (prm->min_links == 0) return "min_links must be at least 1";
    if (const char* why = twoview_check_inputs(poses && matches && match_counts && points && front_bits, match_cap, point_cap, point_cap)) return why;
    const size_t np = (size_t)n_pairs;
    OUT_NEEDS(out, chain, vslam_chain, np);
    // np * match_cap < 2^48: the element count cannot wrap, and the byte count is compared by division
    OUT_FITS(out, map, double[3], np * match_cap);
    OUT_FITS(out, links, int32_t, np * match_cap);
    OUT_FITS(out, ratios, double, np * match_cap);
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y <=
// 65535) and no size wraps: n_pairs < 2^16, the capacities < 2^32, an element <= 8 bytes.
struct ChainPlan {
    unsigned int fwords;      // ballot words per pair of front_bits
    unsigned int rec_blocks;  // grid.x of k_chain_link, k_chain_ratio and k_chain_map
    unsigned int link_pairs;  // n_pairs - 1: grid.y of k_chain_link, grid.x of k_chain_median (0: neither is launched)
    size_t table_elems;       // scratch: the link table, uint32 [link_pairs][point_cap]
    size_t key_elems;         // scratch: the ratio keys, uint64 [link_pairs][match_cap]
    size_t pair_elems;        // scratch: the usable counts (uint32) and the medians (f64), [n_pairs] each
};

inline ChainPlan chain_plan(uint32_t match_cap, uint32_t point_cap, int n_pairs) {
    const TwoViewPlan tv = twoview_plan(match_cap, n_pairs);
    ChainPlan p{};
    p.fwords = tv.fwords, p.rec_blocks = tv.rec_blocks;
    const LinkTable lt = link_table(point_cap, n_pairs);
    p.link_pairs = lt.link_pairs, p.table_elems = lt.elems;
    p.key_elems = (size_t)p.link_pairs * match_cap;
    p.pair_elems = (size_t)n_pairs;
    return p;
}

}  // namespace vslam
