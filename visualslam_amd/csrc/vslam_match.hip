// Descriptor matching of the C ABI (include/vslam.h): argument checks, scratch and launches of kernels_match.hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_match.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_match_plan.h"

using namespace vslam;

int vslam::enqueue_desc_norms(vslam_ctx* c, const vslam_desc_sets& S, int n_pairs, float* norms) {
    LAUNCH(c, "k_desc_norms", k_desc_norms, dim3((unsigned int)(((size_t)S.cap + 255) / 256), n_pairs), dim3(256), S, norms);
    return VSLAM_OK;
}

extern "C" {

int vslam_match_dev(vslam_ctx* c, const vslam_desc_sets* Q, const vslam_desc_sets* T, int n_pairs, float ratio2, int same_octave,
                    const vslam_match_out* out) {
    static_assert(sizeof(vslam_nn2) == 12 && sizeof(vslam_match) == 12 && sizeof(MatchPart) == 12, "record layouts");
    ARGCHK(c, Q && T && out, "match: null argument");
    ARGCHK(c, out->struct_size == sizeof(vslam_match_out), "match: out->struct_size is not sizeof(vslam_match_out)");
    ARGCHK(c, n_pairs >= 0 && n_pairs <= 65535, "match: 0 .. 65535 pairs per call");
    ARGCHK(c, std::isfinite(ratio2) && ratio2 > 0.0f, "match: ratio2 must be finite and positive");
    const char* why = match_check_sets(Q, T, same_octave ? "same_octave needs the points of both sets" : nullptr);
    if (!why) why = match_check_out(out, n_pairs, Q->cap);
    if (why) return fail(c, VSLAM_ERR_INVALID, std::string("match: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const MatchPlan pl = match_plan(Q->cap, T->cap, n_pairs);  // (the counts live on the device: the grid is sized from the capacities)
    float *qnorm = nullptr, *tnorm = nullptr;
    MatchPart* part = nullptr;
    vslam_nn2* nn_ws = nullptr;
    unsigned long long* flags = nullptr;
    unsigned int* chunk_ws = nullptr;
    WsPlan ws;
    ws.add(qnorm, pl.q_elems);
    ws.add(tnorm, pl.t_elems);
    ws.add(part, pl.part_elems);
    if (!out->nn) ws.add(nn_ws, pl.q_elems);
    ws.add(flags, pl.flag_words);
    ws.add(chunk_ws, match_list_ws_elems(pl.fwords, n_pairs));
    TRY(ws.commit(c));
    vslam_nn2* nn = out->nn ? out->nn : nn_ws;

    TRY(enqueue_desc_norms(c, *Q, n_pairs, qnorm));
    TRY(enqueue_desc_norms(c, *T, n_pairs, tnorm));
    const dim3 grid(pl.qtiles, pl.nsplit, n_pairs);
    if (same_octave)
        LAUNCH(c, "k_match_nn2", k_match_nn2<true>, grid, dim3(256), *Q, *T, qnorm, tnorm, (int)pl.nsplit, part);
    else
        LAUNCH(c, "k_match_nn2", k_match_nn2<false>, grid, dim3(256), *Q, *T, qnorm, tnorm, (int)pl.nsplit, part);
    LAUNCH(c, "k_match_merge", k_match_merge, dim3(pl.qrow_blocks, n_pairs), dim3(MT_ROW_WG), *Q, part, (int)pl.nsplit, ratio2, nn, flags, pl.fwords);
    if (out->match_counts) TRY(enqueue_match_list(c, flags, pl.fwords, nn, Q->cap, n_pairs, chunk_ws, out->matches, out->match_cap, out->match_counts));
    return VSLAM_OK;
}

int vslam_match_host(vslam_ctx* c, const float* query, const uint8_t* query_defined, const vslam_point* query_points, size_t nq,
                     const float* train, const uint8_t* train_defined, const vslam_point* train_points, size_t nt, float ratio2,
                     int same_octave, vslam_nn2* nn, vslam_match* matches, size_t match_cap, size_t* n_matches) {
    ARGCHK(c, (query || nq == 0) && (train || nt == 0), "match_host: null descriptors");
    ARGCHK(c, nq < (1u << 31) && nt < (1u << 31) && match_cap < (1u << 31), "match_host: too many rows");
    ARGCHK(c, std::isfinite(ratio2) && ratio2 > 0.0f, "match_host: ratio2 must be finite and positive");
    ARGCHK(c, !same_octave || ((query_points || nq == 0) && (train_points || nt == 0)), "match_host: same_octave needs the points of both sets");
    ARGCHK(c, nn || n_matches, "match_host: no output requested");
    ARGCHK(c, !matches || (n_matches && match_cap > 0), "match_host: matches needs n_matches and a match_cap");
    TRY(usable_ctx(c));

    HostSets hs{{query, train}, {query_defined, train_defined}, {query_points, train_points}, {nq, nt}, nn, matches, match_cap, n_matches};
    DevBufs dev;
    vslam_match_out out{};
    TRY(hs.upload(c, dev, same_octave != 0));
    TRY(hs.outputs(c, dev, out));
    TRY(vslam_match_dev(c, &hs.Q, &hs.T, 1, ratio2, same_octave, &out));
    return hs.download(c, out);
}

}  // extern "C"
