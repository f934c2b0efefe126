// Host driver of the C++ wrapper vslam::buildTracks (visualslam_amd/cxx/vslam_cxx.hpp), for tests/test_tracks_cpu.py and
// tests/test_gpu_tracks.py.  Without an argument it makes the calls that need no GPU - no pairs, and sizes that do not fit -
// and prints "ok".  With "run" it chains three small pairs given by formula (vslam::chainPoses; tests/test_gpu_tracks.py builds
// the same buffers), builds their tracks and prints the bytes of chain, tracks, refs, good_bits and summary in hexadecimal, one
// line each.
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
    const vslam_tracks_params prm{{800.0, 800.0, 960.0, 540.0}, 1e12, 2, 0};
    if (argc < 2 || std::strcmp(argv[1], "run") != 0) {
        const vslam::Tracks none = vslam::buildTracks({}, {}, {}, 8, {}, 8, {}, {}, prm);
        bool refused = false;
        try {
            vslam::buildTracks(std::vector<vslam_pose>(2), std::vector<vslam_match>(16), std::vector<uint32_t>(2), 8, std::vector<uint64_t>(2), 8,
                               std::vector<vslam_chain>(2), std::vector<SLAM::point>(23), prm);  // three frames of 8 points are 24
        } catch (const vslam::Error&) {
            refused = true;
        }
        const bool ok = none.tracks.empty() && none.refs.empty() && none.summary.empty() && refused;
        std::printf(ok ? "ok\n" : "failed\n");
        return ok ? 0 : 1;
    }
    const uint32_t n = 3, cap = 8;
    std::vector<vslam_pose> poses(n);
    std::vector<vslam_match> matches(n * cap);
    std::vector<uint32_t> counts = {8, 5, 8};
    std::vector<double> points(n * cap * 3);
    std::vector<uint64_t> bits = {0xff, 0xf7, 0xff};
    std::vector<SLAM::point> frames((n + 1) * cap);
    for (uint32_t j = 0; j < n; ++j) {
        std::memset(&poses[j], 0, sizeof(vslam_pose));
        const double R[9] = {0.6, 0.0, 0.8, 0.0, 1.0, 0.0, -0.8, 0.0, 0.6};
        std::memcpy(poses[j].R, R, sizeof R);
        poses[j].t[0] = 1.0, poses[j].valid = 1, poses[j].n_matches = counts[j];
        for (uint32_t i = 0; i < cap; ++i) {
            matches[j * cap + i] = vslam_match{(int32_t)i, (int32_t)((i * 3) % 8), 0.0f};
            double* X = &points[(j * cap + i) * 3];
            X[0] = (double)i - 3.0 + 0.25 * j, X[1] = 0.5 * i - 1.0, X[2] = 4.0 + i + j;
        }
    }
    for (uint32_t f = 0; f <= n; ++f)
        for (uint32_t k = 0; k < cap; ++k) frames[f * cap + k] = SLAM::point(100 + 37 * (int)k + 5 * (int)f, 200 + 53 * (int)k - 7 * (int)f, 0, 1, (int)(k % 3), 0);
    const vslam::Trajectory tr = vslam::chainPoses(poses, matches, counts, cap, points, bits, 8, vslam_chain_params{2});
    const vslam::Tracks tk = vslam::buildTracks(poses, matches, counts, cap, bits, 8, tr.chain, frames, prm);
    hex("chain", tr.chain);
    hex("tracks", tk.tracks);
    hex("refs", tk.refs);
    hex("good_bits", tk.goodBits);
    hex("summary", tk.summary);
    return 0;
}
