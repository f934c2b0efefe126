// Guided matching under H or F of the C ABI (include/vslam.h): argument checks and sizing (vslam_guided_hf_plan.h), scratch and
// launches of kernels_match_guided_hf.hip.h; the norms, the merge and the list are the matcher's and the guided pass's
// (vslam_launch.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_match_guided_hf.hip.h"
#include "vslam_ctx.h"
#include "vslam_guided_hf_plan.h"
#include "vslam_launch.h"

using namespace vslam;

extern "C" {

int vslam_match_guided_hf_dev(vslam_ctx* c, const vslam_desc_sets* Q, const vslam_desc_sets* T, const vslam_epipolar* emodels,
                              const vslam_homography* hmodels, int n_pairs, const vslam_guided_hf_params* prm, const vslam_match_out* out) {
    static_assert(sizeof(vslam_guided_hf_params) == 32 && sizeof(GuidedRow) == 32 && sizeof(MatchPart) == 12 && sizeof(GuidedQn) == 8, "record layouts");
    if (const char* why = guided_hf_check_args(Q, T, emodels, hmodels, n_pairs, prm, out)) return fail(c, VSLAM_ERR_INVALID, std::string("match_guided_hf: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const GuidedHfPlan pl = guided_hf_plan(Q->cap, T->cap, n_pairs);
    float *qnorm = nullptr, *tnorm = nullptr;
    GuidedRow *qrows = nullptr, *trows = nullptr;
    MatchPart* part = nullptr;
    vslam_nn2* nn_ws = nullptr;
    unsigned long long* flags = nullptr;
    unsigned int *chunk_ws = nullptr, *kind_list = nullptr;
    WsPlan ws;
    ws.add(qnorm, pl.q_elems);
    ws.add(tnorm, pl.t_elems);
    ws.add(qrows, pl.q_elems);
    ws.add(trows, pl.t_elems);
    ws.add(part, pl.part_elems);
    if (!out->nn) ws.add(nn_ws, pl.q_elems);
    ws.add(flags, pl.flag_words);
    ws.add(chunk_ws, match_list_ws_elems(pl.fwords, n_pairs));
    if (emodels && hmodels) ws.add(kind_list, guided_hf_list_elems(n_pairs));
    TRY(ws.commit(c));
    vslam_nn2* nn = out->nn ? out->nn : nn_ws;

    TRY(enqueue_desc_norms(c, *Q, n_pairs, qnorm));
    TRY(enqueue_desc_norms(c, *T, n_pairs, tnorm));
    LAUNCH(c, "k_guided_hf_rows", k_guided_hf_rows<true>, dim3(pl.qrow_blocks, n_pairs), dim3(MT_ROW_WG), *Q, emodels, hmodels, prm->max_transfer2, qrows);
    LAUNCH(c, "k_guided_hf_rows", k_guided_hf_rows<false>, dim3(pl.trow_blocks, n_pairs), dim3(MT_ROW_WG), *T, emodels, hmodels, prm->max_transfer2, trows);
    // one form of the search per model array given; with both, each form walks its own list of pairs (k_guided_hf_kinds)
    const unsigned int* kind_count = kind_list ? kind_list + 2 * (size_t)n_pairs : nullptr;
    if (kind_list) LAUNCH(c, "k_guided_hf_kinds", k_guided_hf_kinds, dim3(1), dim3(MT_ROW_WG), emodels, hmodels, n_pairs, kind_list, kind_list + 2 * (size_t)n_pairs);
    const dim3 grid(pl.qtiles, pl.nsplit, n_pairs);
    if (emodels) {
        auto k = prm->same_octave ? k_match_guided_hf<true, false> : k_match_guided_hf<false, false>;
        LAUNCH(c, "k_match_guided_hf", k, grid, dim3(256), *Q, *T, qnorm, tnorm, qrows, trows, emodels, hmodels, kind_list, kind_count, prm->max_dist2,
               (int)pl.nsplit, part);
    }
    if (hmodels) {
        auto k = prm->same_octave ? k_match_guided_hf<true, true> : k_match_guided_hf<false, true>;
        LAUNCH(c, "k_match_guided_hf", k, grid, dim3(256), *Q, *T, qnorm, tnorm, qrows, trows, emodels, hmodels, kind_list, kind_count, prm->max_dist2,
               (int)pl.nsplit, part);
    }
    TRY(enqueue_guided_merge(c, *Q, n_pairs, part, pl.nsplit, prm->ratio2, prm->max_desc_dist2, nn, flags, pl.fwords));
    if (out->match_counts)
        TRY(enqueue_match_list(c, flags, pl.fwords, nn, Q->cap, n_pairs, chunk_ws, out->matches, out->match_cap, out->match_counts));
    return VSLAM_OK;
}

int vslam_match_guided_hf_host(vslam_ctx* c, const float* query, const uint8_t* query_defined, const vslam_point* query_points, size_t nq,
                               const float* train, const uint8_t* train_defined, const vslam_point* train_points, size_t nt,
                               const vslam_epipolar* emodel, const vslam_homography* hmodel, const vslam_guided_hf_params* prm, vslam_nn2* nn,
                               vslam_match* matches, size_t match_cap, size_t* n_matches) {
    ARGCHK(c, prm, "match_guided_hf_host: null argument");
    ARGCHK(c, emodel || hmodel, "match_guided_hf_host: epipolar_model and homography_model are both null");
    ARGCHK(c, (query || nq == 0) && (train || nt == 0), "match_guided_hf_host: null descriptors");
    ARGCHK(c, nq < (1u << 31) && nt < (1u << 31) && match_cap < (1u << 31), "match_guided_hf_host: too many rows");
    ARGCHK(c, prm->reserved == 0, "match_guided_hf_host: params->reserved must be 0");
    ARGCHK(c, std::isfinite(prm->ratio2) && prm->ratio2 > 0.0f, "match_guided_hf_host: ratio2 must be finite and positive");
    ARGCHK(c, prm->max_desc_dist2 > 0.0f, "match_guided_hf_host: max_desc_dist2 must be positive (+inf: no bound)");
    ARGCHK(c, !emodel || (std::isfinite(prm->max_dist2) && prm->max_dist2 > 0.0), "match_guided_hf_host: max_dist2 must be finite and positive");
    ARGCHK(c, !hmodel || (std::isfinite(prm->max_transfer2) && prm->max_transfer2 > 0.0), "match_guided_hf_host: max_transfer2 must be finite and positive");
    ARGCHK(c, (query_points || nq == 0) && (train_points || nt == 0), "match_guided_hf_host: the points of both sets are required");
    ARGCHK(c, nn || n_matches, "match_guided_hf_host: no output requested");
    ARGCHK(c, !matches || (n_matches && match_cap > 0), "match_guided_hf_host: matches needs n_matches and a match_cap");
    TRY(usable_ctx(c));

    HostSets hs{{query, train}, {query_defined, train_defined}, {query_points, train_points}, {nq, nt}, nn, matches, match_cap, n_matches};
    DevBufs dev;
    vslam_epipolar* d_emodel = nullptr;
    vslam_homography* d_hmodel = nullptr;
    vslam_match_out out{};
    TRY(hs.upload(c, dev, true));
    if (emodel) TRY(dev.put(c, d_emodel, emodel, 1));
    if (hmodel) TRY(dev.put(c, d_hmodel, hmodel, 1));
    TRY(hs.outputs(c, dev, out));
    TRY(vslam_match_guided_hf_dev(c, &hs.Q, &hs.T, d_emodel, d_hmodel, 1, prm, &out));
    return hs.download(c, out);
}

}  // extern "C"
