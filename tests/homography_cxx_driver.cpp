// Host driver of the C++ wrapper vslam::findHomography (visualslam_amd/cxx/vslam_cxx.hpp), for tests/test_gpu_homography.py.
//   driver pair.bin HYPOTHESES SEED MAX_DIST2 NUM DEN MIN_INLIERS out.bin
// pair.bin: three uint64 (matches, query points, train points), one vslam_epipolar, then the three lists; out.bin: the model,
// the gated epipolar model, one uint64 (inliers) and the inlier records.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vslam_cxx.hpp"

template <typename T>
static bool get(std::FILE* f, T* p, size_t n) {
    return n == 0 || std::fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 9) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n[3];
    vslam_epipolar epi;
    if (!get(f, n, 3) || !get(f, &epi, 1)) return 2;
    std::vector<vslam_match> matches(n[0]);
    std::vector<SLAM::point> qp(n[1]), tp(n[2]);
    if (!get(f, matches.data(), n[0]) || !get(f, qp.data(), n[1]) || !get(f, tp.data(), n[2])) return 2;
    std::fclose(f);
    try {
        const vslam_homography_params prm{(uint32_t)std::strtoul(argv[2], nullptr, 10), (uint32_t)std::strtoul(argv[3], nullptr, 10), std::atof(argv[4]),
                                          (uint32_t)std::strtoul(argv[5], nullptr, 10), (uint32_t)std::strtoul(argv[6], nullptr, 10),
                                          (uint32_t)std::strtoul(argv[7], nullptr, 10)};
        const vslam::Homography r = vslam::findHomography(matches, qp, tp, &epi, prm);
        std::FILE* o = std::fopen(argv[8], "wb");
        if (!o) return 2;
        const uint64_t k = r.inliers.size();
        std::fwrite(&r.model, sizeof r.model, 1, o);
        std::fwrite(&r.gated, sizeof r.gated, 1, o);
        std::fwrite(&k, sizeof k, 1, o);
        if (k) std::fwrite(r.inliers.data(), sizeof(vslam_match), k, o);
        std::fclose(o);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "homography_cxx_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
