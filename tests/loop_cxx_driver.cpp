// Host driver of the C++ wrappers vslam::matchPairs and vslam::verifyLoops (visualslam_amd/cxx/vslam_cxx.hpp), for
// tests/test_loop_cpu.py and tests/test_gpu_loop.py.  Without an argument it makes the calls that the wrappers refuse before they
// need a GPU and prints "ok".  With --valid it makes one small valid matchPairs call and prints "status N": 0 with a GPU, the ABI's
// VSLAM_ERR_HIP without one.
//   driver verify in.bin out.bin   in: uint64 n, cap, c, db_first, min_inliers, num, den, n_hypotheses, seed; counts u32 [n]; desc f32 [n][cap][128];
//                                      defined u8 [n][cap]; points [n][cap]; cand_counts u32 [n]; candidates [n][c]
//                                  out: pairs [n * c]; per slot uint32 count and its matches; models [n * c]; loops [n]; uint32 n_loops and the list
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

int main(int argc, char** argv) {
    const vslam::DescriptorSets two(2, std::vector<std::vector<float>>(3, std::vector<float>(128, 0.5f)));
    const std::vector<vslam_set_pair> table{{1, 0}, {-1, -1}, {0, 0}, {0, 2}};
    if (argc < 2) {
        vslam::DescriptorSets shortRow = two;
        shortRow[1][2].resize(127);
        const vslam::DefinedSets d1(1, std::vector<unsigned char>(3, 1));
        const std::vector<std::vector<SLAM::point>> pts(2, std::vector<SLAM::point>(3)), fewPts(2, std::vector<SLAM::point>(2));
        const std::vector<std::vector<vslam_place_cand>> cands(2), oneList(1);
        bool ok = refused([&] { vslam::matchPairs(shortRow, two, table); }) && refused([&] { vslam::matchPairs(two, shortRow, table); }) &&
                  refused([&] { vslam::matchPairs(two, two, table, 0.0f); }) && refused([&] { vslam::matchPairs(two, two, table, 0.8f, &d1); }) &&
                  refused([&] { vslam::matchPairs(two, two, std::vector<vslam_set_pair>(65536, vslam_set_pair{0, 0})); }) &&
                  refused([&] { vslam::verifyLoops(two, fewPts, cands, 3); }) && refused([&] { vslam::verifyLoops(two, pts, oneList, 3); }) &&
                  refused([&] { vslam::verifyLoops(two, pts, cands, 0); }) && refused([&] { vslam::verifyLoops(two, pts, cands, 9); }) &&
                  refused([&] { vslam::verifyLoops(two, pts, cands, 3, 0, vslam_loop_params{0, 2, 5, 0}); }) &&
                  refused([&] { vslam::verifyLoops(two, pts, cands, 3, 0, vslam_loop_params{12, 2, 0, 0}); }) &&
                  refused([&] { vslam::verifyLoops(two, pts, cands, 3, 0, vslam_loop_params{12, 2, 5, 1}); });
        // no slots: nothing to ask the GPU
        ok = ok && vslam::matchPairs(two, two, std::vector<vslam_set_pair>()).matches.empty();
        std::printf(ok ? "ok\n" : "failed\n");
        return ok ? 0 : 1;
    }
    if (argc == 2 && std::strcmp(argv[1], "--valid") == 0) {
        int status = VSLAM_OK;
        try {
            const vslam::PairMatches r = vslam::matchPairs(two, two, table);
            // equal rows: every query finds row 0 at distance 0 with an equal second, which the ratio test refuses; empty slots stay empty
            if (r.nn.size() != 4 || r.nn[0].size() != 3 || !r.nn[1].empty() || !r.nn[3].empty() || r.nn[2][1].index != 0 || r.nn[2][1].dist2 != 0.0f ||
                !r.matches[0].empty())
                status = 1;
        } catch (const vslam::Error& e) {
            status = e.status;
        }
        std::printf("status %d\n", status);
        return 0;
    }
    if (argc != 4 || std::strcmp(argv[1], "verify") != 0) return 2;
    std::FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 2;
    try {
        uint64_t n[9];
        if (!get(f, n, 9)) return 2;
        const size_t sets = n[0], cap = n[1], c = n[2];
        std::vector<uint32_t> counts(sets), ccounts(sets);
        std::vector<float> desc(sets * cap * 128);
        std::vector<unsigned char> def(sets * cap);
        std::vector<SLAM::point> pts(sets * cap);
        std::vector<vslam_place_cand> cands(sets * c);
        if (!get(f, counts.data(), sets) || !get(f, desc.data(), desc.size()) || !get(f, def.data(), def.size()) || !get(f, pts.data(), pts.size()) ||
            !get(f, ccounts.data(), sets) || !get(f, cands.data(), cands.size()))
            return 2;
        std::fclose(f);
        vslam::DescriptorSets frames(sets);
        vslam::DefinedSets defined(sets);
        std::vector<std::vector<SLAM::point>> points(sets);
        std::vector<std::vector<vslam_place_cand>> candidates(sets);
        for (size_t s = 0; s < sets; ++s) {
            for (size_t r = 0; r < counts[s]; ++r) {
                frames[s].emplace_back(desc.begin() + (s * cap + r) * 128, desc.begin() + (s * cap + r + 1) * 128);
                defined[s].push_back(def[s * cap + r]);
                points[s].push_back(pts[s * cap + r]);
            }
            candidates[s].assign(cands.begin() + s * c, cands.begin() + s * c + std::min<size_t>(ccounts[s], c));
        }
        const vslam::VerifiedLoops v = vslam::verifyLoops(frames, points, candidates, (uint32_t)c, (uint32_t)n[3], vslam_loop_params{(uint32_t)n[4], (uint32_t)n[5], (uint32_t)n[6], 0},
                                                          vslam_epipolar_params{(uint32_t)n[7], (uint32_t)n[8], 4.0}, 0.8f, &defined);
        std::FILE* o = std::fopen(argv[3], "wb");
        if (!o) return 2;
        put(o, v.pairs.data(), v.pairs.size());
        for (const auto& m : v.matches) {
            const uint32_t k = (uint32_t)m.size();
            put(o, &k, 1);
            put(o, m.data(), m.size());
        }
        put(o, v.models.data(), v.models.size());
        put(o, v.loops.data(), v.loops.size());
        const uint32_t k = (uint32_t)v.loopList.size();
        put(o, &k, 1);
        put(o, v.loopList.data(), v.loopList.size());
        std::fclose(o);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "loop_cxx_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
