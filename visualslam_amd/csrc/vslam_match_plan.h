// The host arithmetic that the four matcher entry points share (vslam_match_dev, vslam_match_guided_dev,
// vslam_match_guided_hf_dev, vslam_match_mutual_dev; include/vslam.h) and that needs no HIP: the tiling of the search, the
// grids and scratch sizes, all from the capacities (the counts live on the device), and the checks of the two descriptor sets
// and of the output buffers.  Stated once, here: the kernels take their tile constants from this header
// (kernels_match_common.hip.h), and a host program runs the arithmetic under the sanitizers with extreme capacities
// (tests/guided_plan_driver.cpp, guided_hf_plan_driver.cpp, mutual_plan_driver.cpp).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <initializer_list>

#include "../../include/vslam.h"

namespace vslam {

constexpr int MT_Q = 128;              // query rows per workgroup: 32 per wave
constexpr int MT_T = 64;               // train rows per LDS tile: two 32-column MFMA blocks (and one 64-lane atomic of the reverse table)
constexpr int MT_MAX_SPLIT = 16;       // workgroups that share the train tiles of one query tile
constexpr size_t MT_WANT_WGS = 2048;   // 8 workgroups per compute unit
constexpr unsigned int MT_ROW_WG = 256;  // rows (lanes) per workgroup of the per-row kernels and of the merges

// Grids and scratch of one valid call with n_pairs >= 1.  Every grid dimension stays within HIP's limits (x < 2^31, y and z
// <= 65535) and no size wraps: n_pairs < 2^16, the capacities < 2^32, a scratch record <= 32 bytes, nsplit <= 16.
struct MatchPlan {
    unsigned int qtiles;                    // grid.x of the search: MT_Q-row query tiles
    unsigned int ttiles;                    // MT_T-row train tiles per pair
    unsigned int nsplit;                    // grid.y of the search: the train tiles are dealt round robin to nsplit workgroups
    unsigned int fwords;                    // accepted-query ballot words per pair
    unsigned int qrow_blocks, trow_blocks;  // grid.x of the per-row kernels (and of the merge) over the query / train capacity
    size_t q_elems, t_elems;                // scratch: one record (an f32 norm, a GuidedRow) per query / train row
    size_t part_elems;                      // scratch: one partial result per (pair, split, query row)
    size_t flag_words;                      // scratch: ballot words of all pairs
};

// Train tiles are dealt out round robin to nsplit workgroups per query tile, so that one small pair still fills the chip; the
// merge is exact for any nsplit.
inline MatchPlan match_plan(uint32_t query_cap, uint32_t train_cap, int n_pairs) {
    MatchPlan p{};
    const size_t np = (size_t)n_pairs, qc = query_cap, tc = train_cap;
    p.qtiles = (unsigned int)((qc + MT_Q - 1) / MT_Q);
    p.ttiles = (unsigned int)((tc + MT_T - 1) / MT_T);
    const size_t wgs = (size_t)p.qtiles * np;
    size_t split = (MT_WANT_WGS + wgs - 1) / wgs;
    if (split > (size_t)MT_MAX_SPLIT) split = MT_MAX_SPLIT;
    if (split > p.ttiles) split = p.ttiles;
    p.nsplit = (unsigned int)(split < 1 ? 1 : split);
    p.fwords = (unsigned int)((qc + 63) / 64);
    p.qrow_blocks = (unsigned int)((qc + MT_ROW_WG - 1) / MT_ROW_WG);
    p.trow_blocks = (unsigned int)((tc + MT_ROW_WG - 1) / MT_ROW_WG);
    p.q_elems = np * qc;
    p.t_elems = np * tc;
    p.part_elems = np * p.nsplit * qc;
    p.flag_words = np * p.fwords;
    return p;
}

// The checks of the two descriptor sets, in the entry points' order.  no_points: the message for a set without points where
// the call needs them, nullptr where it does not.
inline const char* match_check_sets(const vslam_desc_sets* Q, const vslam_desc_sets* T, const char* no_points) {
    for (const vslam_desc_sets* s : {Q, T}) {
        if (!s->desc || !s->counts || s->cap == 0) return "a descriptor set needs desc, counts and a capacity";
        if ((reinterpret_cast<uintptr_t>(s->desc) & 15) != 0) return "desc must be 16-byte aligned";
        if (no_points && !s->points) return no_points;
    }
    return nullptr;
}

// The checks of the output buffers (vslam_match_out, vslam_match_mutual_out), in the entry points' order.  other: the call
// has an output of its own besides nn and match_counts; own: what the check of that output, due after nn's, found.
template <typename Out>
inline const char* match_check_out(const Out* out, int n_pairs, uint32_t query_cap, bool other = false, const char* own = nullptr) {
    const size_t np = (size_t)n_pairs;
    if (!out->nn && !other && !out->match_counts) return "no output requested";
    if (out->nn && out->nn_bytes / sizeof(vslam_nn2) < np * query_cap) return "nn buffer too small";
    if (own) return own;
    if (out->matches && (!out->match_counts || out->match_cap == 0)) return "matches needs match_counts and a match_cap";
    if (out->matches && out->matches_bytes / sizeof(vslam_match) < np * out->match_cap) return "matches buffer too small";
    if (out->match_counts && out->match_counts_bytes / sizeof(uint32_t) < np) return "match_counts buffer too small";
    return nullptr;
}

}  // namespace vslam
