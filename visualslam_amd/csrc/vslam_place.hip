// Loop candidates of the C ABI (include/vslam.h, "place recognition"): argument checks (vslam_place_plan.h), scratch and
// launches of kernels_place.hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_place.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_place_plan.h"

using namespace vslam;

extern "C" {

int vslam_place_dev(vslam_ctx* c, const uint32_t* hist_q, uint32_t nq, uint32_t q_first, const uint32_t* hist_db, uint32_t nd, uint32_t db_first,
                    uint32_t K, const vslam_place_params* params, const vslam_place_out* out) {
    static_assert(sizeof(vslam_place_cand) == 12 && sizeof(vslam_place_params) == 24, "record layouts");
    if (const char* why = place_check(hist_q, nq, q_first, hist_db, nd, db_first, K, params, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("place: ") + why);
    TRY(usable_ctx(c));
    if (nq == 0) return VSLAM_OK;

    const PlacePlan pl = place_plan(nq, nd, K);
    uint32_t *weights = out->weights, *self_q = out->self_q, *self_db = out->self_db, *scores = out->scores;
    const bool want_top = out->cand_counts != nullptr, want_scores = out->scores || want_top;
    WsPlan ws;
    if (!weights) ws.add(weights, K);
    if (!self_q) ws.add(self_q, nq);
    if (!self_db) ws.add(self_db, nd);
    if (!scores && want_scores) ws.add(scores, pl.score_elems);
    TRY(ws.commit(c));

    LAUNCH(c, "k_place_df", k_place_df, dim3(pl.df_blocks), dim3(256), hist_db, nd, K, weights);
    LAUNCH(c, "k_place_self", k_place_self, dim3(pl.self_blocks), dim3(64), hist_q, nq, hist_db, K, weights, self_q, self_db);
    if (want_scores && nd > 0)
        LAUNCH(c, "k_place_score", k_place_score, dim3(pl.tiles_d, pl.tiles_q), dim3(256), hist_q, nq, q_first, hist_db, nd, db_first, K, weights,
               params->min_gap, out->scores ? 0 : 1, scores);
    if (want_top)
        LAUNCH(c, "k_place_top", k_place_top, dim3(pl.top_blocks), dim3(64), scores, nd, self_q, self_db, q_first, db_first, *params, out->candidates,
               out->cand_counts);
    return VSLAM_OK;
}

int vslam_place_host(vslam_ctx* c, const uint32_t* hist_q, uint32_t nq, uint32_t q_first, const uint32_t* hist_db, uint32_t nd, uint32_t db_first,
                     uint32_t K, const vslam_place_params* params, const vslam_place_out* out) {
    if (const char* why = place_check(hist_q, nq, q_first, hist_db, nd, db_first, K, params, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("place_host: ") + why);
    TRY(usable_ctx(c));
    if (nq == 0) return VSLAM_OK;  // (as the device call: nothing is written)

    HostMirror hm(c);
    const uint32_t* d_q = hm.in(hist_q, (size_t)nq * K);
    const uint32_t* d_db = hist_db == hist_q && nd == nq ? d_q : hm.in(hist_db, (size_t)nd * K);  // one buffer stays one buffer
    vslam_place_out o{};
    o.struct_size = sizeof(o);
    hm.out(o.candidates, o.candidates_bytes, out->candidates, (size_t)nq * params->max_candidates, true);
    hm.out(o.cand_counts, o.cand_counts_bytes, out->cand_counts, (size_t)nq, false);
    hm.out(o.weights, o.weights_bytes, out->weights, (size_t)K, false);
    hm.out(o.self_q, o.self_q_bytes, out->self_q, (size_t)nq, false);
    hm.out(o.self_db, o.self_db_bytes, out->self_db, (size_t)nd, false);
    hm.out(o.scores, o.scores_bytes, out->scores, (size_t)nq * nd, false);
    TRY(hm.status());
    TRY(vslam_place_dev(c, d_q, nq, q_first, d_db, nd, db_first, K, params, &o));
    return hm.finish();
}

}  // extern "C"
