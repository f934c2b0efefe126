// Host driver of the C++ wrapper vslam::matchGuidedHF (visualslam_amd/cxx/vslam_cxx.hpp), for tests/test_guided_hf_cpu.py and
// tests/test_gpu_guided_hf.py.  Without an argument it makes the calls that the wrapper refuses before it needs a GPU - no
// model, a keypoint list, a descriptor or a defined list of the wrong size - and prints "ok".
//   driver pair.bin MODELS RATIO2 MAX_DESC_DIST2 MAX_DIST2 MAX_TRANSFER2 SAME_OCTAVE out.bin
// pair.bin: two uint64 (query rows, train rows), one vslam_epipolar, one vslam_homography, the query descriptors, the train
// descriptors, the query points, the train points; MODELS: "fh" both records, "f" or "h" that one alone; out.bin: one uint64 and
// the nn records, one uint64 and the match records.  "inf" is a valid bound.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "vslam_cxx.hpp"

template <typename T>
static bool get(std::FILE* f, T* p, size_t n) {
    return n == 0 || std::fread(p, sizeof(T), n, f) == n;
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
    if (argc < 2) {
        const std::vector<std::vector<float>> two(2, std::vector<float>(128, 0.5f)), shortRow(2, std::vector<float>(127, 0.5f));
        const std::vector<SLAM::point> p1(1), p2(2);
        const std::vector<unsigned char> d3(3, 1);
        vslam_epipolar e{};
        vslam_homography h{};
        const vslam_guided_hf_params prm{0.64f, HUGE_VALF, 4.0, 4.0, 0, 0};
        const bool ok = refused([&] { vslam::matchGuidedHF(two, two, p2, p2, nullptr, nullptr); }) &&
                        refused([&] { vslam::matchGuidedHF(two, two, p1, p2, &e, &h); }) && refused([&] { vslam::matchGuidedHF(two, two, p2, p1, nullptr, &h); }) &&
                        refused([&] { vslam::matchGuidedHF(shortRow, two, p2, p2, &e, nullptr); }) &&
                        refused([&] { vslam::matchGuidedHF(two, two, p2, p2, &e, &h, prm, &d3); }) &&
                        refused([&] { vslam::matchGuidedHF(two, two, p2, p2, &e, &h, prm, nullptr, &d3); });
        std::printf(ok ? "ok\n" : "failed\n");
        return ok ? 0 : 1;
    }
    if (argc != 9) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n[2];
    vslam_epipolar e;
    vslam_homography h;
    if (!get(f, n, 2) || !get(f, &e, 1) || !get(f, &h, 1)) return 2;
    std::vector<std::vector<float>> q(n[0], std::vector<float>(128)), t(n[1], std::vector<float>(128));
    std::vector<SLAM::point> qp(n[0]), tp(n[1]);
    for (auto& row : q)
        if (!get(f, row.data(), 128)) return 2;
    for (auto& row : t)
        if (!get(f, row.data(), 128)) return 2;
    if (!get(f, qp.data(), n[0]) || !get(f, tp.data(), n[1])) return 2;
    std::fclose(f);
    try {
        const vslam_guided_hf_params prm{std::strtof(argv[3], nullptr), std::strtof(argv[4], nullptr), std::atof(argv[5]), std::atof(argv[6]), std::atoi(argv[7]), 0};
        const vslam::Matches r = vslam::matchGuidedHF(q, t, qp, tp, std::strchr(argv[2], 'f') ? &e : nullptr, std::strchr(argv[2], 'h') ? &h : nullptr, prm);
        std::FILE* o = std::fopen(argv[8], "wb");
        if (!o) return 2;
        const uint64_t k[2] = {r.nn.size(), r.matches.size()};
        std::fwrite(&k[0], sizeof k[0], 1, o);
        if (k[0]) std::fwrite(r.nn.data(), sizeof(vslam_nn2), k[0], o);
        std::fwrite(&k[1], sizeof k[1], 1, o);
        if (k[1]) std::fwrite(r.matches.data(), sizeof(vslam_match), k[1], o);
        std::fclose(o);
    } catch (const std::exception& ex) {
        std::fprintf(stderr, "guided_hf_cxx_driver: %s\n", ex.what());
        return 1;
    }
    return 0;
}
