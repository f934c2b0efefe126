// Host driver of the C++ wrapper vslam::refitHomography (visualslam_amd/cxx/vslam_cxx.hpp).
//   driver                                                        (tests/test_hrefit_cpu.py) a pair without a model and without
//                                                                 matches: "refused: <what>" when the wrapper throws - there is
//                                                                 no usable HIP device -, "ran: stop 5" when it has one
//   driver pair.bin ROUNDS MAX_DIST2 NUM DEN MIN_INLIERS out.bin  (tests/test_gpu_hrefit.py)
// pair.bin: four uint64 (matches, query points, train points, 1 when an epipolar model follows), one vslam_homography, one
// vslam_epipolar, then the three lists; out.bin: the model, the info record, the gated epipolar model, one uint64 (inliers) and
// the inlier records.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "vslam_cxx.hpp"

template <typename T>
static bool get(std::FILE* f, T* p, size_t n) {
    return n == 0 || std::fread(p, sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
    if (argc == 1) {
        vslam_homography none{};
        none.best = -1;
        try {
            const vslam::HomographyRefit r = vslam::refitHomography(none, {}, {}, {});
            if (r.info.stop != 5 || !r.inliers.empty() || r.model.best != -1) return 1;
            std::printf("ran: stop %d\n", r.info.stop);
        } catch (const vslam::Error& e) {
            std::printf("refused: %s\n", e.what());
        }
        return 0;
    }
    if (argc != 8) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n[4];
    vslam_homography model;
    vslam_epipolar epi;
    if (!get(f, n, 4) || !get(f, &model, 1) || !get(f, &epi, 1)) return 2;
    std::vector<vslam_match> matches(n[0]);
    std::vector<SLAM::point> qp(n[1]), tp(n[2]);
    if (!get(f, matches.data(), n[0]) || !get(f, qp.data(), n[1]) || !get(f, tp.data(), n[2])) return 2;
    std::fclose(f);
    try {
        const vslam_hrefit_params prm{(uint32_t)std::strtoul(argv[2], nullptr, 10), std::atof(argv[3]), (uint32_t)std::strtoul(argv[4], nullptr, 10),
                                      (uint32_t)std::strtoul(argv[5], nullptr, 10), (uint32_t)std::strtoul(argv[6], nullptr, 10)};
        const vslam::HomographyRefit r = vslam::refitHomography(model, matches, qp, tp, prm, n[3] ? &epi : nullptr);
        std::FILE* o = std::fopen(argv[7], "wb");
        if (!o) return 2;
        const uint64_t k = r.inliers.size();
        std::fwrite(&r.model, sizeof r.model, 1, o);
        std::fwrite(&r.info, sizeof r.info, 1, o);
        std::fwrite(&r.gated, sizeof r.gated, 1, o);
        std::fwrite(&k, sizeof k, 1, o);
        if (k) std::fwrite(r.inliers.data(), sizeof(vslam_match), k, o);
        std::fclose(o);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "hrefit_cxx_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
