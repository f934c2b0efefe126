// The host arithmetic of vslam_match_guided_dev (include/vslam.h, "guided matching") that needs no HIP: the argument checks in
// the ABI's order, and the grids and scratch sizes, all from the capacities (the counts and the models live on the device).
// Stated once, here, so that a host program can run it under the sanitizers with extreme capacities
// (tests/guided_plan_driver.cpp).
#pragma once
#include <initializer_list>

#include "vslam_epipolar_plan.h"

namespace vslam {

// One row of the per-row pass (k_guided_rows).  A query row: {a0, a1, a2, a0*a0 + a1*a1}; a train row: {x', y', b0*b0, b1*b1};
// NaN in every field: the row is not trusted (or, on the query side, its pair has no model).
struct __attribute__((aligned(16))) GuidedRow {
    double v[4];
};

// The tiling of the search is k_match_nn2's (kernels_match.hip.h; vslam_match_guided.hip asserts that the two agree).
constexpr unsigned int GUIDED_Q = 128;         // query rows per workgroup
constexpr unsigned int GUIDED_T = 64;          // train rows per LDS tile
constexpr unsigned int GUIDED_MAX_SPLIT = 16;  // workgroups that share the train tiles of one query tile
constexpr size_t GUIDED_WANT_WGS = 2048;       // 8 workgroups per compute unit
constexpr unsigned int GUIDED_ROW_WG = 256;    // rows (lanes) per workgroup of the per-row kernels and of the merge

// The message of the first failed check - the entry point puts "match_guided: " in front -, vslam_match_dev's checks in its
// order with the new ones beside their kind (null, struct_size, n_pairs, the parameters, the sets, the buffers); nullptr: the
// call is valid.
inline const char* guided_check_args(const vslam_desc_sets* Q, const vslam_desc_sets* T, const vslam_epipolar* models, int n_pairs,
                                     const vslam_guided_params* prm, const vslam_match_out* out) {
    if (!Q || !T || !out || !models || !prm) return "null argument";
    if (out->struct_size != sizeof(vslam_match_out)) return "out->struct_size is not sizeof(vslam_match_out)";
    if (n_pairs < 0 || n_pairs > 65535) return "0 .. 65535 pairs per call";
    if (prm->reserved != 0) return "params->reserved must be 0";
    if (!std::isfinite(prm->ratio2) || !(prm->ratio2 > 0.0f)) return "ratio2 must be finite and positive";
    if (!(prm->max_desc_dist2 > 0.0f)) return "max_desc_dist2 must be positive (+inf: no bound)";
    if (const char* why = check_max_dist2(prm->max_dist2)) return why;
    for (const vslam_desc_sets* s : {Q, T}) {
        if (!s->desc || !s->counts || s->cap == 0) return "a descriptor set needs desc, counts and a capacity";
        if ((reinterpret_cast<uintptr_t>(s->desc) & 15) != 0) return "desc must be 16-byte aligned";
        if (!s->points) return "the points of both sets are required";
    }
    const size_t np = (size_t)n_pairs;
    if (!out->nn && !out->match_counts) return "no output requested";
    if (out->nn && out->nn_bytes / sizeof(vslam_nn2) < np * Q->cap) return "nn buffer too small";
    if (out->matches && (!out->match_counts || out->match_cap == 0)) return "matches needs match_counts and a match_cap";
    if (out->matches && out->matches_bytes / sizeof(vslam_match) < np * out->match_cap) return "matches buffer too small";
    if (out->match_counts && out->match_counts_bytes / sizeof(uint32_t) < np) return "match_counts buffer too small";
    return nullptr;
}

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y and z
// <= 65535) and no size wraps: n_pairs < 2^16, the capacities < 2^32, a scratch record <= 32 bytes, nsplit <= 16.
struct GuidedPlan {
    unsigned int qtiles;                // grid.x of k_match_guided: GUIDED_Q-row query tiles
    unsigned int ttiles;                // GUIDED_T-row train tiles per pair
    unsigned int nsplit;                // grid.y of k_match_guided: the train tiles are dealt round robin to nsplit workgroups
    unsigned int fwords;                // accepted-query ballot words per pair
    unsigned int qrow_blocks, trow_blocks;  // grid.x of the per-row kernels (and of the merge) over the query / train capacity
    size_t q_elems, t_elems;            // scratch: one f32 norm and one GuidedRow per query / train row
    size_t part_elems;                  // scratch: one partial result per (pair, split, query row)
    size_t flag_words;                  // scratch: ballot words of all pairs
};

inline GuidedPlan guided_plan(uint32_t query_cap, uint32_t train_cap, int n_pairs) {
    GuidedPlan p{};
    const size_t np = (size_t)n_pairs, qc = query_cap, tc = train_cap;
    p.qtiles = (unsigned int)((qc + GUIDED_Q - 1) / GUIDED_Q);
    p.ttiles = (unsigned int)((tc + GUIDED_T - 1) / GUIDED_T);
    const size_t wgs = (size_t)p.qtiles * np;
    size_t split = (GUIDED_WANT_WGS + wgs - 1) / wgs;
    if (split > GUIDED_MAX_SPLIT) split = GUIDED_MAX_SPLIT;
    if (split > p.ttiles) split = p.ttiles;
    p.nsplit = (unsigned int)(split < 1 ? 1 : split);
    p.fwords = (unsigned int)((qc + 63) / 64);
    p.qrow_blocks = (unsigned int)((qc + GUIDED_ROW_WG - 1) / GUIDED_ROW_WG);
    p.trow_blocks = (unsigned int)((tc + GUIDED_ROW_WG - 1) / GUIDED_ROW_WG);
    p.q_elems = np * qc;
    p.t_elems = np * tc;
    p.part_elems = np * p.nsplit * qc;
    p.flag_words = np * p.fwords;
    return p;
}

}  // namespace vslam
