// The frame structure and loop alignment steps of the C ABI (include/vslam.h, "frame structure" and "loop alignment"):
// argument checks and sizing (vslam_sim3_plan.h), scratch and launches of kernels_sim3.hip.h.  The dense list of usable records
// is the two-view geometry's compaction (enqueue_inlier_list) over {b} records and the slots' m_p.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_sim3.hip.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"
#include "vslam_sim3_plan.h"

using namespace vslam;

namespace {
Sim3SideIn side_in(const vslam_sim3_side* s) {
    return Sim3SideIn{s->cams, s->index, s->map, s->points, s->map_cap, s->point_cap, s->points_cap, s->n_map_pairs, (unsigned int)s->n_frames};
}

// The device copy of one host side (vslam_sim3_host).
vslam_sim3_side mirror_side(HostMirror& m, const vslam_sim3_side* s) {
    vslam_sim3_side d = *s;
    const size_t nf = (size_t)s->n_frames;
    d.cams = m.in(s->cams, nf);
    d.index = m.in(s->index, nf * s->point_cap);
    d.map = m.in(s->map, (size_t)s->n_map_pairs * s->map_cap * 3);
    d.points = m.in(s->points, nf * s->points_cap);
    return d;
}
}  // namespace

extern "C" {

int vslam_frame_world_dev(vslam_ctx* c, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                          const uint64_t* front_bits, uint32_t point_cap, const vslam_chain* chain, int n_pairs, const vslam_frame_world_out* out) {
    static_assert(sizeof(vslam_frame_cam) == 112 && sizeof(vslam_chain) == 176 && sizeof(vslam_pose) == 112 && sizeof(vslam_match) == 12, "record layouts");
    if (const char* why = frame_world_check_args(poses, matches, match_counts, match_cap, front_bits, point_cap, chain, n_pairs, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("frame_world: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const FrameWorldPlan pl = frame_world_plan(match_cap, point_cap, n_pairs);
    const FrameIn in{poses, matches, match_counts, reinterpret_cast<const unsigned long long*>(front_bits), chain, match_cap, pl.fwords, point_cap, n_pairs};
    HIPCHK(c, hipMemsetAsync(out->index, 0xff, pl.index_elems * sizeof(int32_t), c->stream));
    LAUNCH(c, "k_frame_index", k_frame_index, dim3(pl.rec_blocks, n_pairs), dim3(TWOVIEW_REC_WG), in, reinterpret_cast<unsigned int*>(out->index));
    LAUNCH(c, "k_frame_cams", k_frame_cams, dim3(pl.cam_blocks), dim3(FRAME_CAM_WG), poses, chain, n_pairs, out->cams);
    return VSLAM_OK;
}

int vslam_frame_world_host(vslam_ctx* c, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                           const uint64_t* front_bits, uint32_t point_cap, const vslam_chain* chain, int n_pairs, const vslam_frame_world_out* out) {
    if (const char* why = frame_world_check_args(poses, matches, match_counts, match_cap, front_bits, point_cap, chain, n_pairs, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("frame_world_host: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const size_t np = (size_t)n_pairs;
    HostMirror m(c);
    const auto d_poses = m.in(poses, np);
    const auto d_matches = m.in(matches, np * match_cap);
    const auto d_counts = m.in(match_counts, np);
    const auto d_bits = m.in(front_bits, np * twoview_fwords(match_cap));
    const auto d_chain = m.in(chain, np);
    vslam_frame_world_out d{};
    d.struct_size = sizeof(d);
    m.out(d.cams, d.cams_bytes, out->cams, np + 1, false);
    m.out(d.index, d.index_bytes, out->index, (np + 1) * point_cap, false);
    TRY(m.status());
    TRY(vslam_frame_world_dev(c, d_poses, d_matches, d_counts, match_cap, d_bits, point_cap, d_chain, n_pairs, &d));
    return m.finish();
}

int vslam_sim3_dev(vslam_ctx* c, const vslam_sim3_side* query, const vslam_sim3_side* train, const vslam_set_pair* pairs, const vslam_match* matches,
                   const uint32_t* match_counts, uint32_t match_cap, const uint64_t* select_bits, int n_pairs, const vslam_sim3_params* prm,
                   const vslam_sim3_out* out) {
    static_assert(sizeof(vslam_sim3_hyp) == 112 && sizeof(vslam_sim3) == 136 && sizeof(vslam_sim3_corr) == 88 && sizeof(vslam_sim3_side) == 56 &&
                      sizeof(vslam_match) == 12 && sizeof(Sim3Rec) == 80,
                  "record layouts");
    if (const char* why = sim3_check_args(query, train, pairs, matches, match_counts, match_cap, n_pairs, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("sim3: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const unsigned int H = prm->n_hypotheses;
    const Sim3Plan pl = sim3_plan(match_cap, n_pairs, H);
    unsigned int *mcount = nullptr, *ncorr = nullptr, *chunk_ws = nullptr;
    vslam_match *idx = nullptr, *didx = nullptr;
    unsigned long long* uflags = nullptr;
    vslam_sim3_corr* corr_ws = nullptr;
    vslam_sim3_hyp* hyp_ws = nullptr;
    WsPlan ws;
    ws.add(idx, pl.rec_elems);
    ws.add(didx, pl.rec_elems);
    ws.add(uflags, pl.flag_words);
    ws.add(mcount, pl.pair_elems);
    ws.add(ncorr, pl.pair_elems);
    ws.add(chunk_ws, match_list_ws_elems(pl.fwords, n_pairs));
    if (!out->correspondences) ws.add(corr_ws, pl.rec_elems);
    if (!out->hypotheses) ws.add(hyp_ws, pl.hyp_elems);
    TRY(ws.commit(c));
    vslam_sim3_corr* corr = out->correspondences ? out->correspondences : corr_ws;
    vslam_sim3_hyp* hyp = out->hypotheses ? out->hypotheses : hyp_ws;

    const Sim3In in{side_in(query), side_in(train), pairs, matches, match_counts, match_cap, reinterpret_cast<const unsigned long long*>(select_bits),
                    pl.fwords, prm->K};
    const dim3 records(pl.rec_blocks, n_pairs);
    LAUNCH(c, "k_sim3_corr", k_sim3_corr, records, dim3(TWOVIEW_REC_WG), in, idx, uflags, mcount, out->links);
    TRY(enqueue_inlier_list(c, uflags, pl.fwords, idx, mcount, match_cap, n_pairs, chunk_ws, didx, match_cap, ncorr));
    LAUNCH(c, "k_sim3_gather", k_sim3_gather, records, dim3(TWOVIEW_REC_WG), in, didx, ncorr, corr);
    LAUNCH(c, "k_sim3_models", k_sim3_models, dim3(pl.model_blocks, n_pairs), dim3(SIM3_MODEL_WG), corr, ncorr, match_cap, H, prm->seed, hyp);
    LAUNCH(c, "k_sim3_score", k_sim3_score, dim3(pl.score_blocks, pl.nsplit, n_pairs), dim3(EPI_SCORE_WG), corr, ncorr, match_cap, H, pairs, query->cams,
           train->cams, prm->K.fx, prm->K.fy, prm->max_dist2, hyp);
    LAUNCH(c, "k_sim3_select", k_sim3_select, dim3(n_pairs), dim3(256), hyp, mcount, ncorr, match_cap, H, pairs, query->cams,
           (unsigned int)query->n_frames, train->cams, (unsigned int)train->n_frames, out->models);
    if (out->inlier_bits)
        LAUNCH(c, "k_sim3_flags", k_sim3_flags, records, dim3(TWOVIEW_REC_WG), in, out->models, prm->max_dist2,
               reinterpret_cast<unsigned long long*>(out->inlier_bits));
    return VSLAM_OK;
}

int vslam_sim3_host(vslam_ctx* c, const vslam_sim3_side* query, const vslam_sim3_side* train, const vslam_set_pair* pairs, const vslam_match* matches,
                    const uint32_t* match_counts, uint32_t match_cap, const uint64_t* select_bits, int n_pairs, const vslam_sim3_params* prm,
                    const vslam_sim3_out* out) {
    if (const char* why = sim3_check_args(query, train, pairs, matches, match_counts, match_cap, n_pairs, prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("sim3_host: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const size_t np = (size_t)n_pairs, recs = np * match_cap, words = np * twoview_fwords(match_cap), hyps = np * prm->n_hypotheses;
    HostMirror m(c);
    const vslam_sim3_side dq = mirror_side(m, query);
    const bool one = query == train || memcmp(query, train, sizeof(*query)) == 0;  // (the same arrays with the same sizes)
    const vslam_sim3_side dt = one ? dq : mirror_side(m, train);
    const auto d_pairs = m.in(pairs, np);
    const auto d_matches = m.in(matches, recs);
    const auto d_counts = m.in(match_counts, np);
    const auto d_select = m.in(select_bits, words);
    vslam_sim3_out d{};
    d.struct_size = sizeof(d);
    m.out(d.models, d.models_bytes, out->models, np, false);
    m.out(d.inlier_bits, d.inlier_bits_bytes, out->inlier_bits, words, true);
    m.out(d.hypotheses, d.hypotheses_bytes, out->hypotheses, hyps, false);
    m.out(d.correspondences, d.correspondences_bytes, out->correspondences, recs, true);
    m.out(d.links, d.links_bytes, out->links, recs * 2, true);
    TRY(m.status());
    TRY(vslam_sim3_dev(c, &dq, &dt, d_pairs, d_matches, d_counts, match_cap, d_select, n_pairs, prm, &d));
    return m.finish();
}

}  // extern "C"
