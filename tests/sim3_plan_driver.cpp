// Host driver of tests/test_sim3_cpu.py: the argument checks and the grid and scratch sizing of vslam_frame_world_dev and
// vslam_sim3_dev (visualslam_amd/csrc/vslam_sim3_plan.h) without a GPU, built with -fsanitize=address,undefined.  It sweeps
// capacities, pair counts and hypothesis counts up to their extremes and checks, per plan: every grid dimension within HIP's
// limits, the blocks cover the capacities, the tiles are dealt to 1 .. EPI_MAX_SPLIT workgroups, and every scratch size equal to
// its product computed in 128 bits (nothing wrapped).  Then every rejection of the two entry points with its message, over
// pointers it never follows, a buffer one record short for each output, and the order of the checks.
//   driver                  "frames checked=N bad=B first=...", "plan ...", "fargs ..." and "args ..."
//   driver rot in.bin out.bin   in: 3 x 3 f64 matrices; out, per matrix: f64 ok (1 or 0), R [9], n [3] of g3_nearest_rotation
//                               (kernels_geom3.hip.h: the text the kernels compile), for the comparison with tests/sim3ref.py
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels_geom3.hip.h"
#include "plan_driver.h"
#include "vslam_sim3_plan.h"

using namespace vslam;

namespace {
struct Mem {
    vslam_pose poses[1];
    vslam_match matches[1];
    uint32_t counts[1];
    uint64_t bits[1];
    vslam_chain chain[1];
    vslam_frame_cam cams[1];
    int32_t index[1];
    double map[3];
    vslam_point points[1];
    vslam_set_pair pairs[1];
    vslam_sim3 models[1];
};

struct Frames : Mem {  // a valid vslam_frame_world_dev call: 3 pairs of capacity 100, 50 features per frame
    vslam_frame_world_out out{};
    uint32_t match_cap = 100, point_cap = 50;
    int n_pairs = 3;
    const vslam_pose* ps = poses;
    const vslam_match* m = matches;
    const uint32_t* mc = counts;
    const uint64_t* fb = bits;
    const vslam_chain* ch = chain;
    const vslam_frame_world_out* o = &out;
    Frames() {
        out.struct_size = sizeof(out);
        out.cams = cams, out.cams_bytes = 4 * sizeof(vslam_frame_cam);
        out.index = index, out.index_bytes = (size_t)4 * 50 * 4;
    }
    const char* why() const { return frame_world_check_args(ps, m, mc, match_cap, fb, point_cap, ch, n_pairs, o); }
    bool valid() const { return why() == nullptr; }
    bool says(const char* word) const { return why() && std::strstr(why(), word); }
};

struct Call : Mem {  // a valid vslam_sim3_dev call: 3 slots of capacity 70 between two sides
    vslam_sim3_side Q{cams, index, map, points, 100, 50, 60, 4, 5, 0}, T{cams, index, map, points, 90, 40, 30, 7, 8, 0};
    vslam_sim3_params prm{512, 1, 4.0, {800.0, 800.0, 960.0, 540.0}};
    vslam_sim3_out out{};
    uint32_t match_cap = 70;
    int n_pairs = 3;
    const vslam_sim3_side *q = &Q, *t = &T;
    const vslam_set_pair* pr = pairs;
    const vslam_match* m = matches;
    const uint32_t* mc = counts;
    const vslam_sim3_params* p = &prm;
    const vslam_sim3_out* o = &out;
    Call() {
        out.struct_size = sizeof(out);
        out.models = models, out.models_bytes = 3 * sizeof(vslam_sim3);
        out.inlier_bits = bits, out.inlier_bits_bytes = 3 * 2 * 8;
        out.hypotheses = reinterpret_cast<vslam_sim3_hyp*>(matches), out.hypotheses_bytes = (size_t)3 * 512 * sizeof(vslam_sim3_hyp);
        out.correspondences = reinterpret_cast<vslam_sim3_corr*>(matches), out.correspondences_bytes = (size_t)3 * 70 * sizeof(vslam_sim3_corr);
        out.links = index, out.links_bytes = (size_t)3 * 70 * 8;
    }
    const char* why() const { return sim3_check_args(q, t, pr, m, mc, match_cap, n_pairs, p, o); }
    bool valid() const { return why() == nullptr; }
    bool says(const char* word) const { return why() && std::strstr(why(), word); }
};

int rotations(const char* in, const char* out) {
    std::FILE* f = std::fopen(in, "rb");
    if (!f) return 2;
    std::vector<double> rows;
    double M[9];
    while (std::fread(M, sizeof(double), 9, f) == 9) {
        double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, n[3] = {0, 0, 0};
        const bool ok = g3_nearest_rotation(M, R, n);
        rows.push_back(ok ? 1.0 : 0.0);
        rows.insert(rows.end(), R, R + 9);
        rows.insert(rows.end(), n, n + 3);
    }
    std::fclose(f);
    std::FILE* o = std::fopen(out, "wb");
    if (!o) return 2;
    if (!rows.empty()) std::fwrite(rows.data(), sizeof(double), rows.size(), o);
    std::fclose(o);
    return 0;
}
}  // namespace

#define SAYS(T, word, stmt)               \
    {                                     \
        T c;                              \
        stmt;                             \
        args.expect(c.says(word), word);  \
    }

int main(int argc, char** argv) {
    static_assert(sizeof(vslam_frame_cam) == 112 && sizeof(vslam_sim3_hyp) == 112 && sizeof(vslam_sim3) == 136 && sizeof(vslam_sim3_corr) == 88 &&
                      sizeof(vslam_sim3_side) == 56 && sizeof(Sim3Rec) == 80,
                  "record layouts");
    if (argc == 4 && std::strcmp(argv[1], "rot") == 0) return rotations(argv[2], argv[3]);
    if (argc != 1) return 2;
    const uint32_t caps[] = {1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 65535, 65536, 1u << 20, (1u << 31) - 1, 1u << 31, 0xffffff00u, 0xffffff01u, 0xfffffffeu, 0xffffffffu};
    const int pairs[] = {1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 2047, 2048, 2049, 65534, 65535};
    const uint32_t hyps[] = {1, 63, 64, 65, 255, 256, 257, 512, 65534, 65535};
    const unsigned __int128 lim = (unsigned __int128)1 << 63;

    Tally frames;
    for (uint32_t cap : caps)
        for (uint32_t pcap : caps)
            for (int np : pairs) {
                const FrameWorldPlan p = frame_world_plan(cap, pcap, np);
                const unsigned __int128 c = cap, n = (unsigned)np;
                frames.expect((unsigned __int128)p.fwords * 64 >= c && ((unsigned __int128)p.fwords - 1) * 64 < c, "fwords", cap, pcap, np);
                frames.expect((unsigned __int128)p.rec_blocks * TWOVIEW_REC_WG >= c && p.rec_blocks >= 1 && p.rec_blocks < (1u << 31) &&
                                  ((unsigned __int128)p.rec_blocks - 1) * TWOVIEW_REC_WG < c, "rec_blocks", cap, pcap, np);
                frames.expect(p.n_frames == (size_t)np + 1 && np <= 65535, "frames / grid.y", cap, pcap, np);
                frames.expect((unsigned __int128)p.cam_blocks * FRAME_CAM_WG >= n + 1 && ((unsigned __int128)p.cam_blocks - 1) * FRAME_CAM_WG < n + 1 &&
                                  p.cam_blocks <= 1024, "cam_blocks", cap, pcap, np);
                frames.expect((unsigned __int128)p.index_elems == (n + 1) * pcap && (unsigned __int128)p.index_elems * 4 < lim, "index", cap, pcap, np);
            }
    std::printf("frames checked=%ld bad=%ld first=%s\n", frames.checked, frames.bad, frames.first);

    Tally plan;
    for (uint32_t cap : caps)
        for (int np : pairs)
            for (uint32_t nh : hyps) {
                const Sim3Plan p = sim3_plan(cap, np, nh);
                const unsigned __int128 c = cap, n = (unsigned)np;
                plan.expect((unsigned __int128)p.fwords * 64 >= c && ((unsigned __int128)p.fwords - 1) * 64 < c, "fwords", cap, np, nh);
                plan.expect((unsigned __int128)p.rec_blocks * TWOVIEW_REC_WG >= c && p.rec_blocks >= 1 && p.rec_blocks < (1u << 31) &&
                                ((unsigned __int128)p.rec_blocks - 1) * TWOVIEW_REC_WG < c, "rec_blocks", cap, np, nh);
                plan.expect(p.model_blocks >= 1 && p.model_blocks * SIM3_MODEL_WG >= nh && (p.model_blocks - 1) * SIM3_MODEL_WG < nh, "model_blocks", cap, np, nh);
                plan.expect(p.score_blocks >= 1 && p.score_blocks * EPI_SCORE_WG >= nh && (p.score_blocks - 1) * EPI_SCORE_WG < nh, "score_blocks", cap, np, nh);
                plan.expect((unsigned __int128)p.tiles * EPI_TILE >= c && ((unsigned __int128)p.tiles - 1) * EPI_TILE < c, "tiles", cap, np, nh);
                plan.expect(p.nsplit >= 1 && p.nsplit <= EPI_MAX_SPLIT && p.nsplit <= p.tiles, "nsplit", cap, np, nh);
                plan.expect((unsigned __int128)p.rec_elems == n * c && (unsigned __int128)p.rec_elems * sizeof(vslam_sim3_corr) < lim, "records", cap, np, nh);
                plan.expect((unsigned __int128)p.hyp_elems == n * nh && (unsigned __int128)p.hyp_elems * sizeof(vslam_sim3_hyp) < lim, "hyp", cap, np, nh);
                plan.expect((unsigned __int128)p.flag_words == n * p.fwords && (unsigned __int128)p.flag_words * 8 < lim, "flags", cap, np, nh);
                plan.expect(p.pair_elems == (size_t)np && np <= 65535, "pair_elems / grid.y, grid.z", cap, np, nh);
            }
    std::printf("plan checked=%ld bad=%ld first=%s\n", plan.checked, plan.bad, plan.first);

    {
        Tally args;
        {
            Frames c;
            args.expect(c.valid(), "valid");
            c.n_pairs = 1;
            args.expect(c.valid(), "one pair");
            c.n_pairs = 0, c.out.cams_bytes = c.out.index_bytes = 0;
            args.expect(c.valid(), "no pairs: no frames");
            c.n_pairs = 65535, c.match_cap = c.point_cap = 0xffffffffu;  // the largest call
            c.out.cams_bytes = (size_t)65536 * sizeof(vslam_frame_cam), c.out.index_bytes = (size_t)65536 * 0xffffffffu * 4;
            args.expect(c.valid(), "largest");
            c.out.index_bytes -= 1;
            args.expect(c.says("index buffer too small"), "largest index - 1");
            c.out.index_bytes += 1, c.out.cams_bytes -= 1;
            args.expect(c.says("cams buffer too small"), "largest cams - 1");
        }
        SAYS(Frames, "null argument", c.o = nullptr)
        SAYS(Frames, "out->struct_size is not sizeof(vslam_frame_world_out)", c.out.struct_size -= 8)
        SAYS(Frames, "0 .. 65535 pairs per call", c.n_pairs = -1)
        SAYS(Frames, "0 .. 65535 pairs per call", c.n_pairs = 65536)
        SAYS(Frames, "null input", c.ps = nullptr)
        SAYS(Frames, "null input", c.m = nullptr)
        SAYS(Frames, "null input", c.mc = nullptr)
        SAYS(Frames, "null input", c.fb = nullptr)
        SAYS(Frames, "null input", c.ch = nullptr)
        SAYS(Frames, "a capacity is zero", c.match_cap = 0)
        SAYS(Frames, "a capacity is zero", c.point_cap = 0)
        SAYS(Frames, "cams is required", c.out.cams = nullptr)
        SAYS(Frames, "index is required", c.out.index = nullptr)
        SAYS(Frames, "cams buffer too small", c.out.cams_bytes -= sizeof(vslam_frame_cam))
        SAYS(Frames, "cams buffer too small", c.out.cams_bytes -= 1)
        SAYS(Frames, "index buffer too small", c.out.index_bytes -= 4)
        SAYS(Frames, "index buffer too small", c.out.index_bytes -= 1)
        {
            Frames c;  // the order: of two things wrong, the earlier check speaks
            c.out.struct_size -= 8, c.n_pairs = -1;
            args.expect(c.says("struct_size"), "order: struct_size before pairs");
            c.out.struct_size += 8, c.ps = nullptr;
            args.expect(c.says("pairs"), "order: pairs before the inputs");
            c.n_pairs = 3, c.point_cap = 0;
            args.expect(c.says("null input"), "order: null input before the capacities");
            c.ps = c.poses, c.out.cams = nullptr;
            args.expect(c.says("capacity"), "order: capacities before the buffers");
            c.point_cap = 50, c.out.index_bytes = 0;
            args.expect(c.says("cams is required"), "order: cams before index");
        }
        std::printf("fargs checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
        if (args.bad) return 1;
    }

    Tally args;
    {
        Call c;
        args.expect(c.valid(), "valid");
        c.n_pairs = 0;
        args.expect(c.valid(), "no slots");
        c.n_pairs = 1;
        args.expect(c.valid(), "one slot");
        c.n_pairs = 3, c.t = c.q;
        args.expect(c.valid(), "one side on both ends");
        c.out.inlier_bits = nullptr, c.out.hypotheses = nullptr, c.out.correspondences = nullptr, c.out.links = nullptr;
        c.out.inlier_bits_bytes = c.out.hypotheses_bytes = c.out.correspondences_bytes = c.out.links_bytes = 0;
        args.expect(c.valid(), "models alone");
        c.prm.n_hypotheses = 1;
        args.expect(c.valid(), "1 hypothesis");
        c.prm.n_hypotheses = 65535;
        args.expect(c.valid(), "65535 hypotheses");
        c.Q.n_frames = 0, c.Q.n_map_pairs = 1;
        args.expect(c.valid(), "a side without frames");
        c.Q.n_frames = 65536, c.Q.n_map_pairs = 65535;
        args.expect(c.valid(), "a side of 65536 frames");
        c.prm.K.cx = -1e300, c.prm.K.cy = 0.0, c.prm.K.fx = 5e-324;
        args.expect(c.valid(), "extreme intrinsics");
    }
    {
        Call c;
        c.n_pairs = 65535, c.match_cap = 0xffffffffu, c.prm.n_hypotheses = 65535;  // the largest call
        c.Q.map_cap = c.Q.point_cap = c.Q.points_cap = c.T.map_cap = c.T.point_cap = c.T.points_cap = 0xffffffffu;
        c.out.models_bytes = 65535 * sizeof(vslam_sim3);
        c.out.inlier_bits_bytes = (size_t)65535 * (1u << 26) * 8;
        c.out.hypotheses_bytes = (size_t)65535 * 65535 * sizeof(vslam_sim3_hyp);
        c.out.correspondences_bytes = (size_t)65535 * 0xffffffffu * sizeof(vslam_sim3_corr);
        c.out.links_bytes = (size_t)65535 * 0xffffffffu * 8;
        args.expect(c.valid(), "largest");
        c.out.correspondences_bytes -= 1;
        args.expect(c.says("correspondences buffer too small"), "largest correspondences - 1");
        c.out.correspondences_bytes += 1, c.out.inlier_bits_bytes -= 1;
        args.expect(c.says("inlier_bits buffer too small"), "largest bits - 1");
        c.out.inlier_bits_bytes += 1, c.out.hypotheses_bytes -= 1;
        args.expect(c.says("hypotheses buffer too small"), "largest hypotheses - 1");
        c.out.hypotheses_bytes += 1, c.out.models_bytes -= 1;
        args.expect(c.says("models buffer too small"), "largest models - 1");
        c.out.models_bytes += 1, c.out.links_bytes -= 1;
        args.expect(c.says("links buffer too small"), "largest links - 1");
        c.out.links_bytes += 1;
        args.expect(c.valid(), "largest again");
    }
    SAYS(Call, "null argument", c.q = nullptr)
    SAYS(Call, "null argument", c.t = nullptr)
    SAYS(Call, "null argument", c.p = nullptr)
    SAYS(Call, "null argument", c.o = nullptr)
    SAYS(Call, "out->struct_size is not sizeof(vslam_sim3_out)", c.out.struct_size -= 8)
    SAYS(Call, "0 .. 65535 pairs per call", c.n_pairs = -1)
    SAYS(Call, "0 .. 65535 pairs per call", c.n_pairs = 65536)
    SAYS(Call, "1 .. 65535 hypotheses", c.prm.n_hypotheses = 0)
    SAYS(Call, "1 .. 65535 hypotheses", c.prm.n_hypotheses = 65536)
    SAYS(Call, "1 .. 65535 hypotheses", c.prm.n_hypotheses = 0xffffffffu)
    SAYS(Call, "max_dist2 must be finite and positive", c.prm.max_dist2 = 0.0)
    SAYS(Call, "max_dist2 must be finite and positive", c.prm.max_dist2 = -4.0)
    SAYS(Call, "max_dist2 must be finite and positive", c.prm.max_dist2 = std::nan(""))
    SAYS(Call, "max_dist2 must be finite and positive", c.prm.max_dist2 = HUGE_VAL)
    SAYS(Call, "fx and fy must be positive", c.prm.K.fx = 0.0)
    SAYS(Call, "fx and fy must be positive", c.prm.K.fy = -800.0)
    SAYS(Call, "an intrinsic is not finite", c.prm.K.fx = std::nan(""))
    SAYS(Call, "an intrinsic is not finite", c.prm.K.fy = HUGE_VAL)
    SAYS(Call, "an intrinsic is not finite", c.prm.K.cx = std::nan(""))
    SAYS(Call, "an intrinsic is not finite", c.prm.K.cy = -HUGE_VAL)
    SAYS(Call, "a side with a null pointer", c.Q.cams = nullptr)
    SAYS(Call, "a side with a null pointer", c.Q.index = nullptr)
    SAYS(Call, "a side with a null pointer", c.T.map = nullptr)
    SAYS(Call, "a side with a null pointer", c.T.points = nullptr)
    SAYS(Call, "a side with a zero capacity", c.Q.map_cap = 0)
    SAYS(Call, "a side with a zero capacity", c.T.point_cap = 0)
    SAYS(Call, "a side with a zero capacity", c.T.points_cap = 0)
    SAYS(Call, "0 .. 65536 frames per side", c.Q.n_frames = -1)
    SAYS(Call, "0 .. 65536 frames per side", c.T.n_frames = 65537)
    SAYS(Call, "1 .. 65535 map pairs per side", c.Q.n_map_pairs = 0)
    SAYS(Call, "1 .. 65535 map pairs per side", c.T.n_map_pairs = 65536)
    SAYS(Call, "a side's reserved field is not 0", c.T.reserved = 1)
    SAYS(Call, "null input", c.pr = nullptr)
    SAYS(Call, "null input", c.m = nullptr)
    SAYS(Call, "null input", c.mc = nullptr)
    SAYS(Call, "a capacity is zero", c.match_cap = 0)
    SAYS(Call, "models is required", c.out.models = nullptr)
    // a buffer one record short, for each output
    SAYS(Call, "models buffer too small", c.out.models_bytes -= sizeof(vslam_sim3))
    SAYS(Call, "models buffer too small", c.out.models_bytes -= 1)
    SAYS(Call, "inlier_bits buffer too small", c.out.inlier_bits_bytes -= 8)
    SAYS(Call, "inlier_bits buffer too small", c.out.inlier_bits_bytes -= 1)
    SAYS(Call, "hypotheses buffer too small", c.out.hypotheses_bytes -= sizeof(vslam_sim3_hyp))
    SAYS(Call, "hypotheses buffer too small", c.out.hypotheses_bytes -= 1)
    SAYS(Call, "correspondences buffer too small", c.out.correspondences_bytes -= sizeof(vslam_sim3_corr))
    SAYS(Call, "correspondences buffer too small", c.out.correspondences_bytes -= 1)
    SAYS(Call, "links buffer too small", c.out.links_bytes -= 8)
    SAYS(Call, "links buffer too small", c.out.links_bytes -= 1)
    {
        // the header's order: of two things wrong, the earlier check speaks
        Call c;
        c.out.struct_size -= 8, c.n_pairs = -1;
        args.expect(c.says("struct_size"), "order: struct_size before pairs");
        c.out.struct_size += 8, c.prm.n_hypotheses = 0;
        args.expect(c.says("pairs"), "order: pairs before hypotheses");
        c.n_pairs = 3, c.prm.max_dist2 = 0.0;
        args.expect(c.says("hypotheses"), "order: hypotheses before max_dist2");
        c.prm.n_hypotheses = 512, c.prm.K.cx = HUGE_VAL;
        args.expect(c.says("max_dist2"), "order: max_dist2 before the intrinsics");
        c.prm.max_dist2 = 4.0, c.prm.K.fx = 0.0;
        args.expect(c.says("not finite"), "order: finite before positive");
        c.prm.K.cx = 960.0, c.Q.cams = nullptr;
        args.expect(c.says("positive"), "order: the intrinsics before the sides");
        c.prm.K.fx = 800.0, c.T.map_cap = 0;
        args.expect(c.says("null pointer"), "order: the query side before the train side");
        c.Q.cams = c.cams, c.m = nullptr;
        args.expect(c.says("zero capacity"), "order: the sides before the lists");
        c.T.map_cap = 90, c.match_cap = 0;
        args.expect(c.says("null input"), "order: null input before the capacity");
        c.m = c.matches, c.out.models = nullptr;
        args.expect(c.says("a capacity is zero"), "order: the capacity before the buffers");
        c.match_cap = 70, c.out.inlier_bits_bytes = 0;
        args.expect(c.says("models is required"), "order: models before inlier_bits");
        c.out.models = c.models, c.out.hypotheses_bytes = 0;
        args.expect(c.says("inlier_bits buffer"), "order: inlier_bits before hypotheses");
        c.out.inlier_bits_bytes = 3 * 2 * 8, c.out.correspondences_bytes = 0;
        args.expect(c.says("hypotheses buffer"), "order: hypotheses before correspondences");
        c.out.hypotheses_bytes = (size_t)3 * 512 * sizeof(vslam_sim3_hyp), c.out.links_bytes = 0;
        args.expect(c.says("correspondences buffer"), "order: correspondences before links");
    }
    std::printf("args checked=%ld bad=%ld first=%s\n", args.checked, args.bad, args.first);
    return frames.bad || plan.bad || args.bad ? 1 : 0;
}
