// The trajectory step of the C ABI (include/vslam.h, "trajectory"): argument checks and sizing (vslam_chain_plan.h), scratch
// and launches of kernels_chain.hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_chain.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_chain_plan.h"

using namespace vslam;

int vslam::enqueue_chain_link(vslam_ctx* c, const StructLists& L, unsigned int* prev) {
    const ChainPlan pl = chain_plan(L.match_cap, L.point_cap, L.n_pairs);
    const ChainIn in{L.poses, L.matches, L.match_counts, nullptr, reinterpret_cast<const unsigned long long*>(L.front_bits), L.match_cap, pl.fwords,
                     L.point_cap};
    HIPCHK(c, hipMemsetAsync(prev, 0xff, pl.table_elems * sizeof(unsigned int), c->stream));
    LAUNCH(c, "k_chain_link", k_chain_link, dim3(pl.rec_blocks, pl.link_pairs), dim3(CHAIN_REC_WG), in, prev);
    return VSLAM_OK;
}

extern "C" {

int vslam_chain_dev(vslam_ctx* c, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                    const double* points, const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain_params* prm,
                    const vslam_chain_out* out) {
    static_assert(sizeof(vslam_chain) == 176 && sizeof(vslam_pose) == 112 && sizeof(vslam_match) == 12, "record layouts");
    if (const char* why = chain_check_args(poses, matches, match_counts, match_cap, points, front_bits, point_cap, n_pairs, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("chain: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const ChainPlan pl = chain_plan(match_cap, point_cap, n_pairs);
    unsigned int *prev = nullptr, *usable = nullptr;
    unsigned long long* keys = nullptr;
    double* median = nullptr;
    WsPlan ws;
    ws.add(prev, pl.table_elems);
    ws.add(keys, pl.key_elems);
    ws.add(usable, pl.pair_elems);
    ws.add(median, pl.pair_elems);
    TRY(ws.commit(c));

    const ChainIn in{poses, matches, match_counts, points, reinterpret_cast<const unsigned long long*>(front_bits), match_cap, pl.fwords, point_cap};
    const dim3 records(pl.rec_blocks, n_pairs);
    HIPCHK(c, hipMemsetAsync(usable, 0, pl.pair_elems * sizeof(unsigned int), c->stream));
    if (pl.link_pairs) TRY(enqueue_chain_link(c, StructLists{poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs}, prev));
    if (pl.link_pairs || out->links || out->ratios)  // (pair 0 alone has no ratios: only its rows of links and ratios to write)
        LAUNCH(c, "k_chain_ratio", k_chain_ratio, records, dim3(CHAIN_REC_WG), in, prev, keys, usable, out->links, out->ratios);
    if (pl.link_pairs)
        LAUNCH(c, "k_chain_median", k_chain_median, dim3(pl.link_pairs), dim3(CHAIN_MEDIAN_WG), keys, match_counts, match_cap, usable, median);
    LAUNCH(c, "k_chain_walk", k_chain_walk, dim3(1), dim3(1), poses, usable, median, n_pairs, prm->min_links, out->chain);
    if (out->map) LAUNCH(c, "k_chain_map", k_chain_map, records, dim3(CHAIN_REC_WG), in, out->chain, out->map);
    return VSLAM_OK;
}

int vslam_chain_host(vslam_ctx* c, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                     const double* points, const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain_params* prm,
                     const vslam_chain_out* out) {
    if (const char* why = chain_check_args(poses, matches, match_counts, match_cap, points, front_bits, point_cap, n_pairs, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("chain_host: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const size_t np = (size_t)n_pairs, recs = np * match_cap, words = np * twoview_fwords(match_cap);
    HostMirror m(c);
    const auto d_poses = m.in(poses, np);
    const auto d_matches = m.in(matches, recs);
    const auto d_counts = m.in(match_counts, np);
    const auto d_points = m.in(points, recs * 3);
    const auto d_bits = m.in(front_bits, words);
    vslam_chain_out d{};
    d.struct_size = sizeof(d);
    m.out(d.chain, d.chain_bytes, out->chain, np, false);
    m.out(d.map, d.map_bytes, out->map, recs * 3, true);
    m.out(d.links, d.links_bytes, out->links, recs, true);
    m.out(d.ratios, d.ratios_bytes, out->ratios, recs, true);
    TRY(m.status());
    TRY(vslam_chain_dev(c, d_poses, d_matches, d_counts, match_cap, d_points, d_bits, point_cap, n_pairs, prm, &d));
    return m.finish();
}

}  // extern "C"
