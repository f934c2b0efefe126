// Pose from homography of the C ABI (include/vslam.h): argument checks and sizing (vslam_hpose_plan.h), scratch and launches
// of kernels_hpose.hip.h.  The coordinate scratch is the two-view geometry's (enqueue_epi_coords).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_hpose.hip.h"
#include "vslam_ctx.h"
#include "vslam_hpose_plan.h"
#include "vslam_launch.h"

using namespace vslam;

extern "C" {

int vslam_hpose_dev(vslam_ctx* c, const vslam_homography* models, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                    const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap, int n_pairs,
                    const vslam_pose* priors, const vslam_hpose_params* prm, const vslam_hpose_out* out) {
    static_assert(sizeof(vslam_hpose_cand) == 128 && sizeof(vslam_hpose) == 144 && sizeof(vslam_hpose_params) == 64 && sizeof(vslam_pose) == 112 &&
                      sizeof(vslam_homography) == 168 && sizeof(EpiXY) == 32,
                  "record layouts");
    if (const char* why = hpose_check_args(models, matches, match_counts, match_cap, query_points, query_cap, train_points, train_cap, n_pairs, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("hpose: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const HposePlan pl = hpose_plan(match_cap, n_pairs);
    EpiXY* xy = nullptr;
    vslam_hpose_cand* cand_ws = nullptr;
    double* invd = nullptr;
    WsPlan ws;
    ws.add(xy, pl.coords_elems);
    ws.add(invd, pl.invd_elems);
    if (!out->candidates) ws.add(cand_ws, pl.cand_elems);
    TRY(ws.commit(c));
    vslam_hpose_cand* cand = out->candidates ? out->candidates : cand_ws;

    TRY(enqueue_epi_coords(c, matches, match_counts, match_cap, query_points, query_cap, train_points, train_cap, n_pairs, xy));
    LAUNCH(c, "k_hpose_candidates", k_hpose_candidates, dim3(pl.pair_blocks), dim3(HPOSE_PAIR_WG), models, *prm, n_pairs, match_counts, match_cap, cand,
           invd, out->info);
    LAUNCH(c, "k_hpose_vote", k_hpose_vote, dim3(pl.rec_blocks, n_pairs), dim3(HPOSE_REC_WG), xy, match_counts, match_cap, models, prm->K, prm->max_dist2,
           cand, out->info);
    LAUNCH(c, "k_hpose_select", k_hpose_select, dim3(pl.pair_blocks), dim3(HPOSE_PAIR_WG), models, cand, invd, priors, match_counts, match_cap, n_pairs,
           prm->ambiguous_num, prm->ambiguous_den, prm->only_degenerate, out->info, out->poses);
    if (out->points || out->front_bits)
        LAUNCH(c, "k_hpose_points", k_hpose_points, dim3(pl.rec_blocks, n_pairs), dim3(HPOSE_REC_WG), xy, match_counts, match_cap, models, out->poses,
               prm->K, prm->max_dist2, prm->only_degenerate, out->points, reinterpret_cast<unsigned long long*>(out->front_bits), pl.fwords);
    return VSLAM_OK;
}

int vslam_hpose_host(vslam_ctx* c, const vslam_homography* models, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                     const vslam_point* query_points, uint32_t query_cap, const vslam_point* train_points, uint32_t train_cap, int n_pairs,
                     const vslam_pose* priors, const vslam_hpose_params* prm, const vslam_hpose_out* out) {
    if (const char* why = hpose_check_args(models, matches, match_counts, match_cap, query_points, query_cap, train_points, train_cap, n_pairs, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("hpose_host: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const size_t np = (size_t)n_pairs, recs = np * match_cap, words = np * twoview_fwords(match_cap);
    HostMirror m(c);
    const auto d_models = m.in(models, np);
    const auto d_matches = m.in(matches, recs);
    const auto d_counts = m.in(match_counts, np);
    const auto d_q = m.in(query_points, np * query_cap);
    const auto d_t = m.in(train_points, np * train_cap);
    const auto d_priors = m.in(priors, np);
    vslam_hpose_out d{};
    d.struct_size = sizeof(d);
    m.out(d.poses, d.poses_bytes, out->poses, np, true);
    m.out(d.info, d.info_bytes, out->info, np, false);
    m.out(d.candidates, d.candidates_bytes, out->candidates, np * 4, false);
    m.out(d.points, d.points_bytes, out->points, recs * 3, true);
    m.out(d.front_bits, d.front_bits_bytes, out->front_bits, words, true);
    TRY(m.status());
    TRY(vslam_hpose_dev(c, d_models, d_matches, d_counts, match_cap, d_q, query_cap, d_t, train_cap, n_pairs, d_priors, prm, &d));
    return m.finish();
}

}  // extern "C"
