// The host arithmetic of vslam_epipolar_dev (include/vslam.h, "two-view geometry") that needs no HIP: the argument checks in
// the ABI's order, and the grids and scratch sizes, all from the capacities (the counts live on the device).  Stated once,
// here, so that a host program can run it under the sanitizers with extreme capacities (tests/epipolar_plan_driver.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/vslam.h"

namespace vslam {

struct __attribute__((aligned(16))) EpiXY {  // one record of the coordinate scratch: query (x, y), train (u, v); NaN: not trusted
    double x, y, u, v;
};
// The 3 x 3 blocks of a model, as a lane keeps them in registers and the refits' scratch carries them (kernels_estimate.hip.h).
struct EpiModel {
    double F[9];
};
struct HomModel {
    double H[9], G[9];
};

constexpr unsigned int EPI_TILE = 256;      // match records a k_epi_score workgroup stages in LDS at a time (8 KiB)
constexpr unsigned int EPI_SCORE_WG = 256;  // hypotheses (lanes) per k_epi_score workgroup
constexpr unsigned int EPI_MODEL_WG = 64;   // hypotheses per k_epi_models workgroup: one wave, 72 f64 of LDS per lane
constexpr unsigned int EPI_MAX_SPLIT = 64;  // workgroups that share the records of one (pair, hypothesis block)
constexpr size_t EPI_WANT_WGS = 2048;       // 8 workgroups per compute unit

// What vslam_pose_plan.h shares with this header: the sizes that follow from the match capacity alone, and the checks of the
// pair count and of the input lists (`inputs`: every input pointer of the stage is there).
constexpr unsigned int TWOVIEW_REC_WG = 256;  // match records (lanes) per workgroup of the kernels that walk the records
struct TwoViewPlan {
    unsigned int fwords, rec_blocks;  // per pair: ballot words, and TWOVIEW_REC_WG-record blocks (grid.x of the kernels that walk the records)
    size_t coords_elems;              // scratch: {x, y, x', y'} f64 records
};
inline size_t twoview_fwords(size_t match_cap) { return (match_cap + 63) / 64; }
inline TwoViewPlan twoview_plan(uint32_t match_cap, int n_pairs) {
    return {(unsigned int)twoview_fwords(match_cap), (unsigned int)(((size_t)match_cap + TWOVIEW_REC_WG - 1) / TWOVIEW_REC_WG), (size_t)n_pairs * match_cap};
}
inline const char* twoview_check_pairs(int n_pairs) { return n_pairs < 0 || n_pairs > 65535 ? "0 .. 65535 pairs per call" : nullptr; }
inline const char* twoview_check_inputs(bool inputs, uint32_t match_cap, uint32_t query_cap, uint32_t train_cap) {
    return !inputs ? "null input" : match_cap == 0 || query_cap == 0 || train_cap == 0 ? "a capacity is zero" : nullptr;
}

// The checks and sizes that more than one stage's plan header states, once.
inline const char* check_max_dist2(double max_dist2) {
    return !std::isfinite(max_dist2) || !(max_dist2 > 0.0) ? "max_dist2 must be finite and positive" : nullptr;
}
// `not_finite`: the stage's wording of the first message ("an intrinsic is not finite" in the resection stages).
inline const char* check_intrinsics(const vslam_pose_params& K, const char* not_finite = "the intrinsics must be finite") {
    if (!std::isfinite(K.fx) || !std::isfinite(K.fy) || !std::isfinite(K.cx) || !std::isfinite(K.cy)) return not_finite;
    return !(K.fx > 0.0) || !(K.fy > 0.0) ? "fx and fy must be positive" : nullptr;
}
// An output of `out` that is there holds n elements of T (the byte count is compared by division: n may be anything below
// 2^64); OUT_NEEDS: an output the stage cannot do without.  Both return from the *_check_args that uses them.
#define OUT_FITS(out, field, T, n) \
    if ((out)->field && (out)->field##_bytes / sizeof(T) < (n)) return #field " buffer too small"
#define OUT_NEEDS(out, field, T, n)                   \
    if (!(out)->field) return #field " is required"; \
    OUT_FITS(out, field, T, n)
// The list outputs that the `out` of every stage over match records has (epipolar, refit, homography, hrefit), in the ABI's order.
template <class Out>
inline const char* twoview_check_lists(const Out* out, size_t np, size_t fwords) {
    OUT_FITS(out, inlier_bits, uint64_t, np * fwords);
    if (out->inliers && (!out->inlier_counts || out->inlier_cap == 0)) return "inliers needs inlier_counts and an inlier_cap";
    OUT_FITS(out, inliers, vslam_match, np * out->inlier_cap);
    OUT_FITS(out, inlier_counts, uint32_t, np);
    return nullptr;
}
// The link table of enqueue_chain_link (vslam_launch.h): row j - 1 links pair j to pair j - 1.
struct LinkTable {
    unsigned int link_pairs;  // n_pairs - 1: grid.y of k_chain_link (0: not launched)
    size_t elems;             // uint32 [link_pairs][point_cap]
};
inline LinkTable link_table(uint32_t point_cap, int n_pairs) { return {(unsigned int)n_pairs - 1, (size_t)((unsigned int)n_pairs - 1) * point_cap}; }

// The message of the first failed check - the entry point puts its stage in front ("epipolar: ") -, in the order of vslam_match_dev's
// (null, struct_size, n_pairs, the parameters, the inputs, the buffers); nullptr: the call is valid.
inline const char* epipolar_check_args(const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap, const vslam_point* query_points,
                                       uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap, int n_pairs,
                                       const vslam_epipolar_params* prm, const vslam_epipolar_out* out) {
    if (!prm || !out) return "null argument";
    if (out->struct_size != sizeof(vslam_epipolar_out)) return "out->struct_size is not sizeof(vslam_epipolar_out)";
    if (const char* why = twoview_check_pairs(n_pairs)) return why;
    if (prm->n_hypotheses < 1 || prm->n_hypotheses > 65535) return "1 .. 65535 hypotheses";
    if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    if (const char* why = twoview_check_inputs(matches && match_counts && query_points && train_points, match_cap, query_cap, train_cap)) return why;
    const size_t np = (size_t)n_pairs, fwords = twoview_fwords(match_cap);
    OUT_NEEDS(out, models, vslam_epipolar, np);
    if (const char* why = twoview_check_lists(out, np, fwords)) return why;
    OUT_FITS(out, hypotheses, vslam_epipolar_hyp, np * prm->n_hypotheses);
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y and z
// <= 65535) and no size wraps: n_pairs < 2^16, the capacities < 2^32, a record <= 80 bytes.
struct EpipolarPlan : TwoViewPlan {       // (rec_blocks: grid.x of k_epi_coords and k_epi_flags)
    unsigned int model_blocks;            // grid.x of k_epi_models
    unsigned int score_blocks;            // grid.x of k_epi_score: hypothesis blocks
    unsigned int tiles;                   // record tiles per pair
    unsigned int nsplit;                  // grid.y of k_epi_score: the tiles are dealt round robin to nsplit workgroups
    size_t hyp_elems;                     // scratch when the caller gives no hypotheses buffer
    size_t flag_words;                    // scratch when the caller gives no inlier_bits buffer
};

inline EpipolarPlan epipolar_plan(uint32_t match_cap, int n_pairs, uint32_t n_hypotheses) {
    EpipolarPlan p{};
    static_cast<TwoViewPlan&>(p) = twoview_plan(match_cap, n_pairs);
    const size_t np = (size_t)n_pairs;
    p.model_blocks = (n_hypotheses + EPI_MODEL_WG - 1) / EPI_MODEL_WG;
    p.score_blocks = (n_hypotheses + EPI_SCORE_WG - 1) / EPI_SCORE_WG;
    p.tiles = (unsigned int)(((size_t)match_cap + EPI_TILE - 1) / EPI_TILE);
    const size_t wgs = np * p.score_blocks;
    size_t split = (EPI_WANT_WGS + wgs - 1) / wgs;
    if (split > EPI_MAX_SPLIT) split = EPI_MAX_SPLIT;
    if (split > p.tiles) split = p.tiles;
    p.nsplit = (unsigned int)(split < 1 ? 1 : split);
    p.hyp_elems = np * n_hypotheses;
    p.flag_words = np * p.fwords;
    return p;
}

}  // namespace vslam
