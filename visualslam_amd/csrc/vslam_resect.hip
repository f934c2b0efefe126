// The resection step of the C ABI (include/vslam.h, "resection"): argument checks and sizing (vslam_resect_plan.h), scratch
// and launches of kernels_resect.hip.h.  The link table is the trajectory's (enqueue_chain_link), the dense list of usable
// records the two-view geometry's compaction (enqueue_inlier_list) over {b, a} records.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_resect.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_resect_plan.h"

using namespace vslam;

extern "C" {

int vslam_resect_dev(vslam_ctx* c, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                     const double* points, const uint64_t* front_bits, uint32_t point_cap, const vslam_match* obs_matches,
                     const uint32_t* obs_counts, uint32_t obs_cap, const vslam_point* train_points, uint32_t train_cap, int n_pairs,
                     const vslam_resect_params* prm, const vslam_resect_out* out) {
    static_assert(sizeof(vslam_resect_hyp) == 104 && sizeof(vslam_resect) == 120 && sizeof(vslam_resect_corr) == 48 && sizeof(vslam_pose) == 112 &&
                      sizeof(vslam_match) == 12 && sizeof(ResYuv) == 40,
                  "record layouts");
    if (const char* why = resect_check_args(poses, matches, match_counts, match_cap, points, front_bits, point_cap, obs_matches, obs_counts, obs_cap,
                                            train_points, train_cap, n_pairs, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("resect: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const unsigned int H = prm->n_hypotheses;
    const ResectPlan pl = resect_plan(match_cap, point_cap, obs_cap, n_pairs, H);
    unsigned int *prev = nullptr, *ncorr = nullptr, *chunk_ws = nullptr;
    vslam_match *idx = nullptr, *didx = nullptr;
    unsigned long long* uflags = nullptr;
    vslam_resect_corr* corr_ws = nullptr;
    vslam_resect_hyp* hyp_ws = nullptr;
    WsPlan ws;
    ws.add(prev, pl.table_elems);
    ws.add(idx, pl.rec_elems);
    ws.add(didx, pl.rec_elems);
    ws.add(uflags, pl.flag_words);
    ws.add(ncorr, pl.pair_elems);
    ws.add(chunk_ws, match_list_ws_elems(pl.fwords, n_pairs));
    if (!out->correspondences) ws.add(corr_ws, pl.rec_elems);
    if (!out->hypotheses) ws.add(hyp_ws, pl.hyp_elems);
    TRY(ws.commit(c));
    vslam_resect_corr* corr = out->correspondences ? out->correspondences : corr_ws;
    vslam_resect_hyp* hyp = out->hypotheses ? out->hypotheses : hyp_ws;

    const ResIn in{poses, points, match_cap, point_cap, obs_matches, obs_counts, obs_cap, train_points, train_cap, prm->K};
    const dim3 records(pl.rec_blocks, n_pairs);
    if (pl.link_pairs) TRY(enqueue_chain_link(c, StructLists{poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs}, prev));
    LAUNCH(c, "k_res_corr", k_res_corr, records, dim3(TWOVIEW_REC_WG), in, prev, idx, uflags, pl.fwords, out->links);
    TRY(enqueue_inlier_list(c, uflags, pl.fwords, idx, obs_counts, obs_cap, n_pairs, chunk_ws, didx, obs_cap, ncorr));
    LAUNCH(c, "k_res_gather", k_res_gather, records, dim3(TWOVIEW_REC_WG), in, didx, ncorr, corr);
    LAUNCH(c, "k_res_models", k_res_models, dim3(pl.model_blocks, n_pairs), dim3(RES_MODEL_WG), corr, ncorr, obs_cap, H, prm->seed, hyp);
    LAUNCH(c, "k_res_score", k_res_score, dim3(pl.score_blocks, pl.nsplit, n_pairs), dim3(EPI_SCORE_WG), corr, ncorr, obs_cap, H, prm->K.fx, prm->K.fy,
           prm->max_dist2, hyp);
    LAUNCH(c, "k_res_select", k_res_select, dim3(n_pairs), dim3(256), hyp, obs_counts, obs_cap, ncorr, H, out->models);
    if (out->inlier_bits)
        LAUNCH(c, "k_res_flags", k_res_flags, records, dim3(TWOVIEW_REC_WG), in, idx, out->models, prm->max_dist2,
               reinterpret_cast<unsigned long long*>(out->inlier_bits), pl.fwords);
    return VSLAM_OK;
}

int vslam_resect_host(vslam_ctx* c, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                      const double* points, const uint64_t* front_bits, uint32_t point_cap, const vslam_match* obs_matches,
                      const uint32_t* obs_counts, uint32_t obs_cap, const vslam_point* train_points, uint32_t train_cap, int n_pairs,
                      const vslam_resect_params* prm, const vslam_resect_out* out) {
    if (const char* why = resect_check_args(poses, matches, match_counts, match_cap, points, front_bits, point_cap, obs_matches, obs_counts, obs_cap,
                                            train_points, train_cap, n_pairs, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("resect_host: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const size_t np = (size_t)n_pairs, recs = np * match_cap, words = np * twoview_fwords(match_cap);
    const size_t orecs = np * obs_cap, owords = np * twoview_fwords(obs_cap), hyps = np * prm->n_hypotheses;
    HostMirror m(c);
    const auto d_poses = m.in(poses, np);
    const auto d_matches = m.in(matches, recs);
    const auto d_counts = m.in(match_counts, np);
    const auto d_points = m.in(points, recs * 3);
    const auto d_bits = m.in(front_bits, words);
    const auto d_obs = m.in(obs_matches, orecs);
    const auto d_ocounts = m.in(obs_counts, np);
    const auto d_train = m.in(train_points, np * train_cap);
    vslam_resect_out d{};
    d.struct_size = sizeof(d);
    m.out(d.models, d.models_bytes, out->models, np, false);
    m.out(d.inlier_bits, d.inlier_bits_bytes, out->inlier_bits, owords, true);
    m.out(d.hypotheses, d.hypotheses_bytes, out->hypotheses, hyps, false);
    m.out(d.correspondences, d.correspondences_bytes, out->correspondences, orecs, true);
    m.out(d.links, d.links_bytes, out->links, orecs, true);
    TRY(m.status());
    TRY(vslam_resect_dev(c, d_poses, d_matches, d_counts, match_cap, d_points, d_bits, point_cap, d_obs, d_ocounts, obs_cap, d_train, train_cap, n_pairs,
                         prm, &d));
    return m.finish();
}

}  // extern "C"
