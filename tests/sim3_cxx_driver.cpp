// Host driver of the C++ wrappers vslam::frameWorld and vslam::alignLoops (visualslam_amd/cxx/vslam_cxx.hpp), for
// tests/test_sim3_cpu.py and tests/test_gpu_sim3.py.  Without an argument it makes the calls that the wrappers refuse before they
// need a GPU and prints "ok".  With --valid it makes one small valid alignLoops call and prints "status N": 0 with a GPU, the ABI's
// VSLAM_ERR_HIP without one.
//   driver run in.bin out.bin   in: uint64 n_slots, match_cap, n_hypotheses, seed, has_select, two_sides; f64 max_dist2, fx, fy, cx, cy;
//                                   per side: uint64 n_frames, point_cap, map_pairs, map_cap, points_cap; cams, index, map, points;
//                                   pairs [n_slots]; matches [n_slots][match_cap]; counts u32 [n_slots]; select u64 [n_slots][words] if has_select
//                               out: models [n_slots]; inlier bits [n_slots][words]; correspondences [n_slots][match_cap]; links [n_slots][match_cap][2]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vslam_cxx.hpp"

template <typename T>
static bool get(std::FILE* f, T* p, size_t n) {
    return n == 0 || std::fread(p, sizeof(T), n, f) == n;
}
template <typename T>
static void put(std::FILE* f, const T* p, size_t n) {
    if (n) std::fwrite(p, sizeof(T), n, f);
}

template <typename F>
static bool refused(F call) {
    try {
        call();
    } catch (const vslam::Error& e) {
        return e.status == VSLAM_ERR_INVALID;
    }
    return false;
}

static vslam::WorldSide smallSide() {  // 3 frames of 4 features over 2 pairs of capacity 5, nothing valid
    vslam::WorldSide s;
    s.frames.cams.assign(3, vslam_frame_cam{});
    s.frames.index.assign(3 * 4, -1);
    s.pointCap = 4, s.mapCap = 5, s.pointsCap = 4;
    s.map.assign(2 * 5 * 3, 0.0);
    s.points.assign(3 * 4, SLAM::point{});
    return s;
}

static bool readSide(std::FILE* f, vslam::WorldSide& s) {
    uint64_t h[5];
    if (!get(f, h, 5)) return false;
    s.frames.cams.resize(h[0]);
    s.frames.index.resize(h[0] * h[1]);
    s.pointCap = (uint32_t)h[1], s.mapCap = (uint32_t)h[3], s.pointsCap = (uint32_t)h[4];
    s.map.resize(h[2] * h[3] * 3);
    s.points.resize(h[0] * h[4]);
    return get(f, s.frames.cams.data(), s.frames.cams.size()) && get(f, s.frames.index.data(), s.frames.index.size()) && get(f, s.map.data(), s.map.size()) &&
           get(f, s.points.data(), s.points.size());
}

int main(int argc, char** argv) {
    const vslam_sim3_params prm{64, 1, 16.0, {800.0, 800.0, 960.0, 540.0}};
    const std::vector<vslam_set_pair> table{{1, 0}, {-1, -1}, {0, 2}};
    const std::vector<vslam_match> matches(3 * 5, vslam_match{0, 0, 0.0f});
    const std::vector<uint32_t> counts(3, 5);
    if (argc < 2) {
        const vslam::WorldSide side = smallSide();
        vslam::WorldSide shortIndex = side, noMap = side, oddMap = side;
        shortIndex.frames.index.pop_back();
        noMap.map.clear();
        oddMap.map.pop_back();
        vslam_sim3_params noHyp = prm, badDist = prm, badK = prm;
        noHyp.n_hypotheses = 0, badDist.max_dist2 = 0.0, badK.K.fx = 0.0;
        const std::vector<uint64_t> sel(3, ~0ull), shortSel(2, ~0ull);
        const std::vector<vslam_pose> poses(2);
        const std::vector<vslam_chain> chain(2), shortChain(1);
        const std::vector<vslam_match> pm(2 * 5);
        const std::vector<uint32_t> pc(2, 0);
        const std::vector<uint64_t> bits(2, 0);
        bool ok = refused([&] { vslam::alignLoops(shortIndex, side, table, matches, counts, 5, prm); }) &&
                  refused([&] { vslam::alignLoops(side, noMap, table, matches, counts, 5, prm); }) &&
                  refused([&] { vslam::alignLoops(side, oddMap, table, matches, counts, 5, prm); }) &&
                  refused([&] { vslam::alignLoops(side, side, table, matches, counts, 4, prm); }) &&
                  refused([&] { vslam::alignLoops(side, side, table, matches, std::vector<uint32_t>(2, 5), 5, prm); }) &&
                  refused([&] { vslam::alignLoops(side, side, table, matches, counts, 5, prm, &shortSel); }) &&
                  refused([&] { vslam::alignLoops(side, side, table, matches, counts, 5, noHyp, &sel); }) &&
                  refused([&] { vslam::alignLoops(side, side, table, matches, counts, 5, badDist); }) &&
                  refused([&] { vslam::alignLoops(side, side, table, matches, counts, 5, badK); }) &&
                  refused([&] { vslam::alignLoops(side, side, std::vector<vslam_set_pair>(65536, vslam_set_pair{0, 0}), matches, counts, 5, prm); }) &&
                  refused([&] { vslam::frameWorld(poses, pm, pc, 5, bits, 4, shortChain); }) &&
                  refused([&] { vslam::frameWorld(poses, pm, pc, 6, bits, 4, chain); });
        // no slots, no pairs: nothing to ask the GPU
        ok = ok && vslam::alignLoops(side, side, {}, {}, {}, 5, prm).models.empty();
        ok = ok && vslam::frameWorld({}, {}, {}, 5, {}, 4, {}).cams.empty();
        std::printf(ok ? "ok\n" : "failed\n");
        return ok ? 0 : 1;
    }
    if (argc == 2 && std::strcmp(argv[1], "--valid") == 0) {
        int status = VSLAM_OK;
        try {
            const vslam::WorldSide side = smallSide();
            const vslam::LoopAlignment r = vslam::alignLoops(side, side, table, matches, counts, 5, prm);
            // no camera is valid: no correspondence, no model; the empty slot has no records and no segments
            if (r.models.size() != 3 || r.models[0].best != -1 || r.models[0].n_matches != 5 || r.models[0].n_corr != 0 || r.models[1].n_matches != 0 ||
                r.models[1].query_segment != -1 || r.models[2].n_valid != 0 || r.links[0] != -1)
                status = 1;
        } catch (const vslam::Error& e) {
            status = e.status;
        }
        std::printf("status %d\n", status);
        return 0;
    }
    if (argc != 4 || std::strcmp(argv[1], "run") != 0) return 2;
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    try {
        uint64_t n[6];
        double d[5];
        if (!get(f, n, 6) || !get(f, d, 5)) return 2;
        vslam::WorldSide q, t;
        if (!readSide(f, q) || (n[5] && !readSide(f, t))) return 2;
        const size_t slots = n[0], cap = n[1], words = slots * ((cap + 63) / 64);
        std::vector<vslam_set_pair> pairs(slots);
        std::vector<vslam_match> mt(slots * cap);
        std::vector<uint32_t> cnt(slots);
        std::vector<uint64_t> select(n[4] ? words : 0);
        if (!get(f, pairs.data(), slots) || !get(f, mt.data(), mt.size()) || !get(f, cnt.data(), slots) || !get(f, select.data(), select.size())) return 2;
        std::fclose(f);
        const vslam_sim3_params p{(uint32_t)n[2], (uint32_t)n[3], d[0], {d[1], d[2], d[3], d[4]}};
        const vslam::LoopAlignment r = vslam::alignLoops(q, n[5] ? t : q, pairs, mt, cnt, (uint32_t)cap, p, n[4] ? &select : nullptr);
        std::FILE* o = std::fopen(argv[3], "wb");
        if (!o) return 2;
        put(o, r.models.data(), r.models.size());
        put(o, r.inlierBits.data(), r.inlierBits.size());
        put(o, r.correspondences.data(), r.correspondences.size());
        put(o, r.links.data(), r.links.size());
        std::fclose(o);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "sim3_cxx_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
