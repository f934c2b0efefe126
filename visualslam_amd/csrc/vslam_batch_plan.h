// The stream and event plan of one chunk of a batch call (vslam_detect_batch_dev, vslam_pyramid_build_u8): on which lane
// each piece of the chunk goes, behind which event, and after which octave it is enqueued.  A pure function of a few
// small values, with no HIP in it, so that tests/batch_plan_driver.cpp sweeps it on the CPU; enqueue_dog and its callers
// (vslam_hip.hip) carry it out and decide nothing of this themselves.
#pragma once
#include "../../include/vslam.h"

namespace vslam {

// Where a piece of a chunk is enqueued: the context's stream or one of its auxiliary streams (vslam_ctx::aux).
enum class Lane : int {
    Main = 0,
    Harris = 1,  // aux[0]: the Harris chain
    List = 2,    // aux[1]: the lattice scans, the list compaction and what follows the list
    Up = 3,      // aux[2]: the second half's upsample of a large batch
};

struct BatchPlanIn {
    int nf = 1;         // frames of the chunk
    int n_octaves = 0;
    bool tiled[VSLAM_MAX_OCTAVES] = {};    // the default path runs the octave LDS-tiled (OctPath::Tile0 / Tile1)
    bool lattice[VSLAM_MAX_OCTAVES] = {};  // the octave has extrema sites (lat_rows > 0 && lat_cols > 0)
    bool scan_ok[VSLAM_MAX_OCTAVES] = {};  // its matrix-core configuration can run the lattice scan inside the octave kernel
    bool up2_ok = false;  // octave 0's matrix-core configuration can form its base from the frame, and the geometry allows it
    bool dog = false, harris = false;
    bool do_extrema = false;  // the lattice scans run at all
    bool lists = false;       // the DoG point lists and their counts are asked for
    bool localize = false, orient = false, extrema_dense = false;
    int extrema_window = 3;
    bool mx = false;                 // the matrix path is on
    bool bases_are_scratch = false;  // nobody reads the octave bases after the call
    bool side = false;               // the call has side streams (BatchFork::side)
    bool capturing = false;          // a stream capture is on
    bool later_chunk = false;        // not the first chunk of its call: the scratch still has readers from the chunk before
};

struct BatchPlan {
    // The octave whose kernels the held-back side work waits for: the last LDS-tiled one, for batches of 32 frames or
    // more with side streams; -1 = none (batch_plan has the measurements).
    int gate = -1;
    // The Harris chain: enqueued before the DoG path (harris_after < 0), or right behind ev_oct[harris_after].
    Lane harris_lane = Lane::Main;
    int harris_after = -1;
    // Octave oo's lattice scan and list compaction are enqueued once octave after[oo]'s kernels are (after[oo] >= oo, never
    // decreasing); on the list lane the scan waits for ev_oct[after[oo]].
    Lane scan_lane = Lane::Main;
    int after[VSLAM_MAX_OCTAVES] = {};
    bool ev_oct = false;  // every octave's kernels are followed by a record of ev_oct[o]
    // Octave 0's base: formed inside its kernel (up2_fused), or upsampled - frames [0, nf_a) on the main lane and, when
    // nf_a < nf, the rest on up_lane (behind ev_chunk when up_waits_chunk; ev_up2 marks its end).
    bool up2_fused = false;
    int nf_a = 1;
    Lane up_lane = Lane::Main;
    bool up_waits_chunk = false;
    bool ev_chunk = false;  // recorded on the main lane behind the chunk's last octave
    // Matrix path: the lattice scan of octave o runs inside its octave kernel and leaves the site / seam maps.
    bool fused[VSLAM_MAX_OCTAVES] = {};
    bool sitemap = false;    // the maps are needed: some octave of some chunk of the call can be fused
    bool wait_pack = false;  // the previous chunk's readers of the maps are on the list lane: the main lane waits for ev_pack
    // Orientation stage: the edge test of octave 0's records right behind that octave's list (on the Harris lane when
    // forked), and the per-octave launches spread over the list, Harris and upsample lanes.
    bool early_edge = false, early_edge_forked = false, spread = false;
};

inline BatchPlan batch_plan(const BatchPlanIn& in) {
    BatchPlan pl;
    const int n = in.dog ? in.n_octaves : 0;
    // THE CAPTURE RULE.  Under stream capture (hipGraph) no two SIDE streams of the call may wait on each other's events.
    // The topology is legal (fork from the origin stream, cross edges between the forked streams, all joined back) and every event is recorded on
    // a stream that is already part of the capture; but this HIP runtime (ROCm 7.2's libamdhip64.so.7 and the copy torch 2.10
    // bundles alike) never returns from hipStreamEndCapture then: a function that calls itself for every entry of a
    // per-stream vector (the shape of hip::Stream::EndCapture over parallelCaptureStreams_) recurses 174,000 frames deep and
    // the process dies of stack exhaustion - no HIP status is ever seen.  It was reproduced through this library and without
    // it (profiles/r05_graph_try.json, profiles/r05_capture_cycle_repro.txt): two side streams that wait on each other's
    // events are harmless by themselves and fatal as soon as each also waits on an origin-stream event again in between -
    // which this library's side streams do on every octave's event.  The orientation stage has two such pairs - the early
    // edge test (list stream -> Harris stream -> back) and the spread launches (list stream -> two idle side streams ->
    // back); each alone reproduces the crash.  While a capture is on, both stay on the list stream; everything else forks
    // from and joins to the main (origin) stream.
    // This is the one place that derives "side lanes may fork to each other"; both orientation forks read it.
    const bool side_forks = in.side && !in.capturing;

    // Where the side work runs decides how much of the VALU-issue-bound octave kernels it costs
    // (gate: the last LDS-tiled octave, -1 = none; 256 x 1080p, same box):
    //  * the Harris chain (VALU-heavy) always waits for that octave's kernel - it is enqueued right
    //    behind ev_oct[gate], so that nothing enqueued on its stream later can get in front of it -
    //    and runs beside the coarse-octave strip kernels, which are short of waves: k_pyr_octave 7.46 -> 6.06 ms per launch, +1.4 % frames/s;
    //  * the plain extrema scan (HBM-heavy, ~90 VALU instructions per thread) starts as soon as its
    //    octave is written, i.e. octave 0's scan runs beside octave 1's kernel: +2..3 % frames/s
    //    over holding it back as well (the tail after the tiled octaves is as VALU-bound as they are,
    //    so the scan's memory time is what gets hidden);
    //  * the scan with FeaturePointLocalization inside (params.localize, ~8x the instructions) is
    //    held back like the Harris chain: +0.5 % in the localize / orient / describe modes.
    // Small batches keep the eager order: there the chain's latency matters, not the issue slots.
    // (matrix path: starting the Harris chain at once, or behind octave 0 / 2 / 3 instead of 1, moved the step by less than
    // +-1.5 % - 14.54 .. 14.90 ms on one box - so the gate stays where the default path has it)
    if (in.side && in.nf >= 32)
        for (int o = 0; o < n; ++o)
            if (in.tiled[o]) pl.gate = o;
    pl.harris_lane = in.side ? Lane::Harris : Lane::Main;
    pl.harris_after = (in.dog && in.side) ? pl.gate : -1;

    // the scan with FeaturePointLocalization inside is held back like the Harris chain; the plain one is eager
    const int held = (in.side && in.localize) ? pl.gate : -1;
    pl.scan_lane = in.side ? Lane::List : Lane::Main;
    for (int oo = 0; oo < n; ++oo) pl.after[oo] = oo < held ? held : oo;
    pl.ev_oct = in.side;

    // Large batches go through the upsample and octave 0 in two halves: the second half is upsampled
    // on the side stream (idle until octave 0 is done) while the first half's octave-0 kernel runs, so
    // only half of the bandwidth-bound upsample is exposed in front of the VALU-bound octave kernels.
    // The second half goes to a lane of its own (Lane::Up): on the list lane it would queue behind the previous
    // chunk's whole list chain.  It overwrites bases the previous chunk's octave kernels (main stream)
    // read, and nothing else orders it behind them - with pyramid-only outputs there is not even a scan
    // waiting on ev_oct - so it waits for ev_chunk, recorded at the end of every chunk's main-stream work.
    // (quarters and eighths were measured again in round 3 with the side upsample at normal priority: 21.41 /
    // 21.44 ms against 21.29 for halves in the same configuration - no gain)
    // Matrix path, batched entry (the octave bases are scratch nobody reads afterwards): octave 0's kernel forms its base from
    // the frame while it stages a tile (kernels_pyramid_mx.hip.h: mx_stage_tile_up2) - no upsample kernel, no base in HBM.
    pl.up2_fused = in.mx && in.bases_are_scratch && in.up2_ok;
    const bool halves = !pl.up2_fused && in.side && in.nf >= 64;
    pl.nf_a = halves ? in.nf / 2 : in.nf;
    pl.up_lane = halves ? Lane::Up : Lane::Main;
    pl.up_waits_chunk = halves && in.later_chunk;
    pl.ev_chunk = in.side;

    pl.sitemap = in.dog && in.mx && in.do_extrema && !in.localize && !in.extrema_dense && in.extrema_window == 3;
    bool any_fused = false;
    for (int o = 0; o < n; ++o) any_fused |= pl.fused[o] = pl.sitemap && in.lattice[o] && in.scan_ok[o];
    // (the previous chunk of the call had the same flags, and fused[] does not depend on the frame count)
    pl.wait_pack = in.later_chunk && in.side && any_fused;

    pl.early_edge = in.dog && in.orient && n > 1;
    pl.early_edge_forked = pl.early_edge && side_forks;
    pl.spread = in.dog && in.orient && side_forks;
    return pl;
}

}  // namespace vslam
