// The bundle adjustment of the C ABI (include/vslam.h, "bundle adjustment"): argument checks and sizing (vslam_bundle_plan.h),
// scratch and launches of kernels_bundle.hip.h.  The tables are the trajectory's and the tracks stage's (enqueue_chain_link,
// enqueue_trk_next).  The number of launches depends on `sweeps` alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/vslam.h"
#include "kernels_bundle.hip.h"
#include "vslam_bundle_plan.h"
#include "vslam_ctx.h"
#include "vslam_launch.h"

using namespace vslam;

extern "C" {

int vslam_bundle_dev(vslam_ctx* c, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                     const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain* chain, const vslam_point* frame_points,
                     const vslam_track* tracks_in, const vslam_track_ref* refs, const vslam_bundle_cam* cams_in, const vslam_bundle_params* prm,
                     const vslam_bundle_out* out) {
    static_assert(sizeof(vslam_bundle_cam) == 160 && sizeof(vslam_bundle_point) == 40 && sizeof(vslam_bundle_params) == 48, "record layouts");
    if (const char* why = bundle_check_args(poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs, chain, frame_points, tracks_in, refs,
                                            prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("bundle: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const BundlePlan pl = bundle_plan(match_cap, point_cap, n_pairs);
    unsigned int *prev = nullptr, *next = nullptr;
    BaCam* state = nullptr;
    double* partial = nullptr;
    WsPlan ws;
    ws.add(prev, pl.trk.prev_elems);
    ws.add(next, pl.trk.next_elems);
    ws.add(state, pl.state_elems);
    ws.add(partial, pl.partial_elems);
    TRY(ws.commit(c));

    const TrkIn in{poses,     matches,      match_counts, reinterpret_cast<const unsigned long long*>(front_bits), chain, frame_points, match_cap,
                   pl.trk.fwords, point_cap, n_pairs};
    const dim3 records(pl.trk.rec_blocks, n_pairs), rows(pl.sum_blocks, n_pairs), pairs(pl.pair_blocks);
    if (pl.trk.link_pairs) {
        const StructLists L{poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs};
        TRY(enqueue_chain_link(c, L, prev));
        TRY(enqueue_trk_next(c, L, chain, prev, next));
    }
    LAUNCH(c, "k_ba_init", k_ba_init, records, dim3(TRK_REC_WG), in, *prm, prev, next, tracks_in, cams_in, out->tracks, out->point_info, state);
    for (unsigned int sweep = 0; sweep < prm->sweeps; ++sweep) {
        LAUNCH(c, "k_ba_points", k_ba_points, records, dim3(TRK_REC_WG), in, *prm, prev, next, state, out->tracks, out->point_info, sweep);
        for (int which : {BA_CUR, BA_CAND}) {
            LAUNCH(c, "k_ba_cam_pass", k_ba_cam_pass, rows, dim3(REFIT_WG), in, *prm, refs, out->tracks, state, which, partial, pl.sum_blocks);
            LAUNCH(c, "k_ba_cam_step", k_ba_cam_step, pairs, dim3(RR_PAIR_WG), in, partial, pl.sum_blocks, which, sweep, prm->sweeps, state, out->cams);
        }
    }
    LAUNCH(c, "k_ba_cam_pass", k_ba_cam_pass, rows, dim3(REFIT_WG), in, *prm, refs, out->tracks, state, BA_FINAL, partial, pl.sum_blocks);
    LAUNCH(c, "k_ba_cam_step", k_ba_cam_step, pairs, dim3(RR_PAIR_WG), in, partial, pl.sum_blocks, BA_FINAL, prm->sweeps, prm->sweeps, state, out->cams);
    if (out->member_bits)
        LAUNCH(c, "k_ba_member_bits", k_ba_member_bits, records, dim3(TRK_REC_WG), in, *prm, refs, out->tracks, state,
               reinterpret_cast<unsigned long long*>(out->member_bits));
    LAUNCH(c, "k_ba_points_final", k_ba_points_final, records, dim3(TRK_REC_WG), in, *prm, prev, next, state, out->tracks, out->point_info);
    return VSLAM_OK;
}

int vslam_bundle_host(vslam_ctx* c, const vslam_pose* poses, const vslam_match* matches, const uint32_t* match_counts, uint32_t match_cap,
                      const uint64_t* front_bits, uint32_t point_cap, int n_pairs, const vslam_chain* chain, const vslam_point* frame_points,
                      const vslam_track* tracks_in, const vslam_track_ref* refs, const vslam_bundle_cam* cams_in, const vslam_bundle_params* prm,
                      const vslam_bundle_out* out) {
    if (const char* why = bundle_check_args(poses, matches, match_counts, match_cap, front_bits, point_cap, n_pairs, chain, frame_points, tracks_in, refs,
                                            prm, out))
        return fail(c, VSLAM_ERR_INVALID, std::string("bundle_host: ") + why);
    TRY(usable_ctx(c));
    if (n_pairs == 0) return VSLAM_OK;

    const size_t np = (size_t)n_pairs, recs = np * match_cap, words = np * twoview_fwords(match_cap);
    HostMirror m(c);
    const auto d_poses = m.in(poses, np);
    const auto d_matches = m.in(matches, recs);
    const auto d_counts = m.in(match_counts, np);
    const auto d_bits = m.in(front_bits, words);
    const auto d_chain = m.in(chain, np);
    const auto d_frames = m.in(frame_points, (np + 1) * point_cap);
    const auto d_tracks_in = m.in(tracks_in, recs);
    const auto d_refs = m.in(refs, recs);
    const auto d_cams_in = m.in(cams_in, np);  // (optional)
    vslam_bundle_out d{};
    d.struct_size = sizeof(d);
    m.out(d.tracks, d.tracks_bytes, out->tracks, recs, true);
    m.out(d.cams, d.cams_bytes, out->cams, np, false);
    m.out(d.point_info, d.point_info_bytes, out->point_info, recs, true);
    m.out(d.member_bits, d.member_bits_bytes, out->member_bits, 2 * words, true);
    TRY(m.status());
    TRY(vslam_bundle_dev(c, d_poses, d_matches, d_counts, match_cap, d_bits, point_cap, n_pairs, d_chain, d_frames, d_tracks_in, d_refs, d_cams_in, prm, &d));
    return m.finish();
}

}  // extern "C"
