// Mutual matching of the C ABI (include/vslam.h): argument checks and sizing (vslam_mutual_plan.h), scratch and launches of
// kernels_match_mutual.hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_match_mutual.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_mutual_plan.h"

using namespace vslam;

extern "C" {

int vslam_match_mutual_dev(vslam_ctx* c, const vslam_desc_sets* Q, const vslam_desc_sets* T, int n_pairs, float ratio2, int same_octave,
                           const vslam_match_mutual_out* out) {
    static_assert(sizeof(vslam_rnn) == 8 && sizeof(vslam_nn2) == 12 && sizeof(MatchPart) == 12, "record layouts");
    static_assert(MT_T == 64, "one 64-lane atomic of the reverse table per train tile");
    if (const char* why = mutual_check_args(Q, T, n_pairs, ratio2, same_octave, out)) return fail(c, VSLAM_ERR_INVALID, std::string("match_mutual: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const MutualPlan pl = mutual_plan(Q->cap, T->cap, n_pairs);
    float *qnorm = nullptr, *tnorm = nullptr;
    MatchPart* part = nullptr;
    vslam_nn2* nn_ws = nullptr;
    unsigned long long *flags = nullptr, *rev = nullptr;
    unsigned int* chunk_ws = nullptr;
    WsPlan ws;
    ws.add(qnorm, pl.q_elems);
    ws.add(tnorm, pl.t_elems);
    ws.add(part, pl.part_elems);
    if (!out->nn) ws.add(nn_ws, pl.q_elems);
    ws.add(flags, pl.flag_words);
    ws.add(rev, pl.rev_elems);
    ws.add(chunk_ws, match_list_ws_elems(pl.fwords, n_pairs));
    TRY(ws.commit(c));
    vslam_nn2* nn = out->nn ? out->nn : nn_ws;

    HIPCHK(c, hipMemsetAsync(rev, 0xff, pl.rev_bytes, c->stream));  // REV_NONE everywhere: nothing offered yet
    TRY(enqueue_desc_norms(c, *Q, n_pairs, qnorm));
    TRY(enqueue_desc_norms(c, *T, n_pairs, tnorm));
    const dim3 grid(pl.qtiles, pl.nsplit, n_pairs);
    if (same_octave)
        LAUNCH(c, "k_match_nn2_mutual", k_match_nn2_mutual<true>, grid, dim3(256), *Q, *T, qnorm, tnorm, (int)pl.nsplit, part, rev);
    else
        LAUNCH(c, "k_match_nn2_mutual", k_match_nn2_mutual<false>, grid, dim3(256), *Q, *T, qnorm, tnorm, (int)pl.nsplit, part, rev);
    LAUNCH(c, "k_match_mutual_merge", k_match_mutual_merge, dim3(pl.qrow_blocks, n_pairs), dim3(MT_ROW_WG), *Q, part, (int)pl.nsplit, ratio2, rev, T->cap,
           nn, flags, pl.fwords);
    if (out->rnn) LAUNCH(c, "k_match_rnn_write", k_match_rnn_write, dim3(pl.trow_blocks, n_pairs), dim3(MT_ROW_WG), *T, rev, out->rnn);
    if (out->match_counts)
        TRY(enqueue_match_list(c, flags, pl.fwords, nn, Q->cap, n_pairs, chunk_ws, out->matches, out->match_cap, out->match_counts));
    return VSLAM_OK;
}

int vslam_match_mutual_host(vslam_ctx* c, const float* query, const uint8_t* query_defined, const vslam_point* query_points, size_t nq,
                            const float* train, const uint8_t* train_defined, const vslam_point* train_points, size_t nt, float ratio2,
                            int same_octave, vslam_nn2* nn, vslam_rnn* rnn, vslam_match* matches, size_t match_cap, size_t* n_matches) {
    ARGCHK(c, (query || nq == 0) && (train || nt == 0), "match_mutual_host: null descriptors");
    ARGCHK(c, nq < (1u << 31) && nt < (1u << 31) && match_cap < (1u << 31), "match_mutual_host: too many rows");
    ARGCHK(c, std::isfinite(ratio2) && ratio2 > 0.0f, "match_mutual_host: ratio2 must be finite and positive");
    ARGCHK(c, !same_octave || ((query_points || nq == 0) && (train_points || nt == 0)), "match_mutual_host: same_octave needs the points of both sets");
    ARGCHK(c, nn || rnn || n_matches, "match_mutual_host: no output requested");
    ARGCHK(c, !matches || (n_matches && match_cap > 0), "match_mutual_host: matches needs n_matches and a match_cap");
    TRY(usable_ctx(c));

    HostSets hs{{query, train}, {query_defined, train_defined}, {query_points, train_points}, {nq, nt}, nn, matches, match_cap, n_matches};
    DevBufs dev;
    vslam_match_mutual_out out{};
    TRY(hs.upload(c, dev, same_octave != 0));
    TRY(hs.outputs(c, dev, out));
    if (rnn) {
        TRY(dev.get(c, out.rnn, nt));
        out.rnn_bytes = std::max<size_t>(nt, 1) * sizeof(vslam_rnn);
    }
    TRY(vslam_match_mutual_dev(c, &hs.Q, &hs.T, 1, ratio2, same_octave, &out));
    return hs.download(c, out, rnn, out.rnn, nt * sizeof(vslam_rnn));
}

}  // extern "C"
