// Host driver of the C++ wrapper vslam::refitFundamental (visualslam_amd/cxx/vslam_cxx.hpp), for tests/test_gpu_refit.py.
//   driver pair.bin ROUNDS MAX_DIST2 out.bin
// pair.bin: three uint64 (matches, query points, train points), one vslam_epipolar, then the three lists; out.bin: the model,
// the info record, one uint64 (inliers) and the inlier records.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vslam_cxx.hpp"

template <typename T>
static bool get(std::FILE* f, T* p, size_t n) {
    return n == 0 || std::fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc != 5) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n[3];
    vslam_epipolar model;
    if (!get(f, n, 3) || !get(f, &model, 1)) return 2;
    std::vector<vslam_match> matches(n[0]);
    std::vector<SLAM::point> qp(n[1]), tp(n[2]);
    if (!get(f, matches.data(), n[0]) || !get(f, qp.data(), n[1]) || !get(f, tp.data(), n[2])) return 2;
    std::fclose(f);
    try {
        const vslam::Refit r = vslam::refitFundamental(model, matches, qp, tp, vslam_refit_params{(uint32_t)std::atoi(argv[2]), std::atof(argv[3])});
        std::FILE* o = std::fopen(argv[4], "wb");
        if (!o) return 2;
        const uint64_t k = r.inliers.size();
        std::fwrite(&r.model, sizeof r.model, 1, o);
        std::fwrite(&r.info, sizeof r.info, 1, o);
        std::fwrite(&k, sizeof k, 1, o);
        if (k) std::fwrite(r.inliers.data(), sizeof(vslam_match), k, o);
        std::fclose(o);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "refit_cxx_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
