// The host arithmetic of vslam_frame_world_dev and vslam_sim3_dev (include/vslam.h, "frame structure" and "loop alignment")
// that needs no HIP: the argument checks in the ABI's order, and the grids and scratch sizes, all from the capacities (the
// counts and the tables live on the device).  Stated once, here, so that a host program can run it under the sanitizers with
// extreme capacities (tests/sim3_plan_driver.cpp).  The walk over the correspondences has the shape of vslam_epipolar_dev's -
// lane = hypothesis, tiles of EPI_TILE records dealt round robin to nsplit workgroups - so those grids are epipolar_plan's.
#pragma once
#include "vslam_epipolar_plan.h"

namespace vslam {

constexpr unsigned int FRAME_CAM_WG = 64;    // frames (lanes) per k_frame_cams workgroup
constexpr unsigned int SIM3_MODEL_WG = 64;   // hypotheses per k_sim3_models workgroup: one wave, everything in registers

struct __attribute__((aligned(8))) Sim3Rec {  // what k_sim3_score stages of one correspondence: 80 bytes, 20 KiB per tile
    double X[3], Y[3], uq, vq, ut, vt;
};

// ---- frame structure ----

// The message of the first failed check, without the stage in front, in the order of vslam_chain_dev's (null, struct_size,
// n_pairs, the inputs, the buffers); nullptr: the call is valid.
inline const char* frame_world_check_args(const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                                          const uint64_t* front_bits, uint32_t point_cap, const vslam_chain* chain, int n_pairs,
                                          const vslam_frame_world_out* out) {
    if (!out) return "null argument";
    if (out->struct_size != sizeof(vslam_frame_world_out)) return "out->struct_size is not sizeof(vslam_frame_world_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (const char* why = twoview_check_inputs(poses && matches && match_counts && front_bits && chain, match_cap, point_cap, point_cap)) return why;
    const size_t nf = n_pairs ? (size_t)n_pairs + 1 : 0;  // (no frame without a pair: nothing is written)
    OUT_NEEDS(out, cams, vslam_frame_cam, nf);
    // nf * point_cap < 2^49: the element count cannot wrap, and the byte count is compared by division
    OUT_NEEDS(out, index, int32_t, nf * point_cap);
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y <=
// 65535): the record walk is over the n_pairs <= 65535 pairs - pair j fills frame j's row and, where it is the source, frame
// j + 1's -, so the 65536 frames of the largest call never become a grid dimension.
struct FrameWorldPlan {
    unsigned int fwords;      // ballot words per pair of front_bits
    unsigned int rec_blocks;  // grid.x of k_frame_index
    unsigned int cam_blocks;  // grid.x of k_frame_cams
    size_t n_frames;
    size_t index_elems;       // int32 [n_frames][point_cap]: preset to -1 before k_frame_index
};

inline FrameWorldPlan frame_world_plan(uint32_t match_cap, uint32_t point_cap, int n_pairs) {
    const TwoViewPlan tv = twoview_plan(match_cap, n_pairs);
    FrameWorldPlan p{};
    p.fwords = tv.fwords, p.rec_blocks = tv.rec_blocks;
    p.n_frames = (size_t)n_pairs + 1;
    p.cam_blocks = (unsigned int)((p.n_frames + FRAME_CAM_WG - 1) / FRAME_CAM_WG);
    p.index_elems = p.n_frames * point_cap;
    return p;
}

// ---- loop alignment ----

inline const char* sim3_check_side(const vslam_sim3_side* s) {
    if (!s->cams || !s->index || !s->map || !s->points) return "a side with a null pointer";
    if (s->map_cap == 0 || s->point_cap == 0 || s->points_cap == 0) return "a side with a zero capacity";
    if (s->n_frames < 0 || s->n_frames > 65536) return "0 .. 65536 frames per side";
    if (s->n_map_pairs < 1 || s->n_map_pairs > 65535) return "1 .. 65535 map pairs per side";
    if (s->reserved != 0) return "a side's reserved field is not 0";
    return nullptr;
}

// The message of the first failed check, without the stage in front, in the order of vslam_resect_dev's (null, struct_size,
// n_pairs, the parameters, the inputs, the buffers); nullptr: the call is valid.
inline const char* sim3_check_args(const vslam_sim3_side* query, const vslam_sim3_side* train, const vslam_set_pair* pairs, const vslam_match* matches,
                                   const uint32_t* match_counts, uint32_t match_cap, int n_pairs, const vslam_sim3_params* prm,
                                   const vslam_sim3_out* out) {
    if (!query || !train || !prm || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_sim3_out)) return "out->struct_size is not sizeof(vslam_sim3_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (prm->n_hypotheses < 1 || prm->n_hypotheses > 65535) return "1 .. 65535 hypotheses";
    if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    if (const char* why = check_intrinsics(prm->K, "an intrinsic is not finite")) return why;
    if (const char* why = sim3_check_side(query)) return why;
    if (const char* why = sim3_check_side(train)) return why;
    if (!pairs || !matches || !match_counts) return "null input";
    if (match_cap == 0) return "a capacity is zero";
    const size_t np = (size_t)n_pairs, fwords = twoview_fwords(match_cap);
    OUT_NEEDS(out, models, vslam_sim3, np);
    // np * match_cap < 2^48 and np * n_hypotheses < 2^32: no element count wraps, and the byte counts are compared by division
    OUT_FITS(out, inlier_bits, uint64_t, np * fwords);
    OUT_FITS(out, hypotheses, vslam_sim3_hyp, np * prm->n_hypotheses);
    OUT_FITS(out, correspondences, vslam_sim3_corr, np * match_cap);
    OUT_FITS(out, links, int32_t[2], np * match_cap);
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y and z
// <= 65535) and no size wraps: n_pairs < 2^16, n_hypotheses < 2^16, match_cap < 2^32, a record <= 112 bytes - below 2^56.
struct Sim3Plan : EpipolarPlan {  // over match_cap: fwords, rec_blocks (k_sim3_corr, k_sim3_gather, k_sim3_flags), model_blocks,
                                  // score_blocks, tiles, nsplit, hyp_elems, flag_words (the usable words)
    size_t rec_elems;             // scratch: {b} per record, its dense list, and the dense correspondences: [n_pairs][match_cap] each
    size_t pair_elems;            // scratch: m_p and n_corr, uint32 [n_pairs] each
};

inline Sim3Plan sim3_plan(uint32_t match_cap, int n_pairs, uint32_t n_hypotheses) {
    static_assert(SIM3_MODEL_WG == EPI_MODEL_WG, "model_blocks is epipolar_plan's");
    Sim3Plan p{};
    static_cast<EpipolarPlan&>(p) = epipolar_plan(match_cap, n_pairs, n_hypotheses);
    p.rec_elems = (size_t)n_pairs * match_cap;
    p.pair_elems = (size_t)n_pairs;
    return p;
}

}  // namespace vslam
