// Host driver of the C++ wrapper vslam::resectPoses (visualslam_amd/cxx/vslam_cxx.hpp), for tests/test_gpu_resect.py.  Without an
// argument it makes the calls that need no GPU - no pairs, and sizes that do not fit - and prints "ok".  With "run" it resects
// two small pairs given by formula and table (tests/test_gpu_resect.py builds the same buffers) and prints the bytes of models,
// inlier bits, correspondences and links in hexadecimal, one line each.
#include <cstdio>
#include <cstring>

#include "vslam_cxx.hpp"

template <typename T>
static void hex(const char* name, const std::vector<T>& v) {
    std::printf("%s ", name);
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) std::printf("%02x", p[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    const vslam_resect_params prm{64, 3, 4.0, {800.0, 800.0, 960.0, 540.0}};
    if (argc < 2 || std::strcmp(argv[1], "run") != 0) {
        const vslam::Resection none = vslam::resectPoses({}, {}, {}, 8, {}, {}, 8, {}, {}, 8, {}, 8, prm);
        bool refused = false;
        try {
            vslam::resectPoses(std::vector<vslam_pose>(2), std::vector<vslam_match>(16), std::vector<uint32_t>(2), 8, std::vector<double>(48),
                               std::vector<uint64_t>(2), 8, std::vector<vslam_match>(15), std::vector<uint32_t>(2), 8, std::vector<SLAM::point>(16), 8, prm);
        } catch (const vslam::Error&) {
            refused = true;
        }
        std::printf(none.models.empty() && none.links.empty() && refused ? "ok\n" : "failed\n");
        return none.models.empty() && refused ? 0 : 1;
    }
    const uint32_t n = 2, cap = 8;
    const int cols[8] = {1740, 1943, 2096, 2223, 2270, 2638, 2577, 2858}, rows[8] = {622, 1046, 1382, 836, 1126, 1535, 953, 1256};
    const double depth[8] = {6.0, 9.5, 7.0, 8.0, 10.5, 6.5, 9.0, 7.5};
    std::vector<vslam_pose> poses(n);
    std::vector<vslam_match> matches(n * cap);
    std::vector<uint32_t> counts = {8, 8};
    std::vector<double> points(n * cap * 3);
    std::vector<uint64_t> bits = {0xff, 0xff};
    std::vector<SLAM::point> train(n * cap);
    for (uint32_t j = 0; j < n; ++j) {
        std::memset(&poses[j], 0, sizeof(vslam_pose));
        poses[j].R[0] = poses[j].R[4] = poses[j].R[8] = 1.0;
        poses[j].t[0] = 1.0, poses[j].valid = 1, poses[j].n_matches = 8;
        for (uint32_t i = 0; i < cap; ++i) {
            matches[j * cap + i] = vslam_match{(int32_t)i, (int32_t)i, 0.0f};
            double* X = &points[(j * cap + i) * 3];
            X[0] = ((double)i - 3.5) * 0.7, X[1] = ((double)((i * 3) % 8) - 3.5) * 0.5, X[2] = depth[i];
            train[j * cap + i] = SLAM::point(rows[i], cols[i], 0, 0, 0, 0);
        }
    }
    const vslam::Resection rs = vslam::resectPoses(poses, matches, counts, cap, points, bits, 8, matches, counts, cap, train, cap, prm);
    hex("models", rs.models);
    hex("bits", rs.inlierBits);
    hex("correspondences", rs.correspondences);
    hex("links", rs.links);
    return 0;
}
