// Host driver of the C++ wrapper vslam::refineResection (visualslam_amd/cxx/vslam_cxx.hpp), for tests/test_resect_refine_cpu.py
// and tests/test_gpu_resect_refine.py.  Without an argument it makes the calls that need no GPU - no pairs, and sizes that do not
// fit - and prints "ok".  With "run" it refines two small pairs given by formula (tests/test_gpu_resect_refine.py builds the same
// buffers) and prints the bytes of models, info and inlier bits in hexadecimal, one line each.
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
    const vslam_resect_refine_params prm{8, 1e30, {800.0, 800.0, 960.0, 540.0}};
    if (argc < 2 || std::strcmp(argv[1], "run") != 0) {
        const vslam::RefinedResection none = vslam::refineResection({}, {}, 8, prm);
        bool refused = false;
        try {
            vslam::refineResection(std::vector<vslam_resect>(2), std::vector<vslam_resect_corr>(15), 8, prm);
        } catch (const vslam::Error&) {
            refused = true;
        }
        const bool ok = none.models.empty() && none.info.empty() && none.inlierBits.empty() && refused;
        std::printf(ok ? "ok\n" : "failed\n");
        return ok ? 0 : 1;
    }
    // every number below is a short binary fraction: the Python side builds the same bytes
    const uint32_t n = 2, cap = 24;
    std::vector<vslam_resect> models(n);
    std::vector<vslam_resect_corr> rows(n * cap);
    for (uint32_t j = 0; j < n; ++j) {
        std::memset(&models[j], 0, sizeof(vslam_resect));
        models[j].R[0] = models[j].R[4] = models[j].R[8] = 1.0;
        models[j].t[0] = 0.5, models[j].t[1] = -0.125 * (double)j;
        models[j].n_obs = cap, models[j].n_corr = cap - 3 * j, models[j].best = (int32_t)j, models[j].n_valid = 7;
        for (uint32_t i = 0; i < cap; ++i) {
            vslam_resect_corr& c = rows[j * cap + i];
            std::memset(&c, 0, sizeof c);
            c.Y[0] = ((double)(i % 5) - 2.0) * 0.75, c.Y[1] = ((double)((i * 3) % 7) - 3.0) * 0.5, c.Y[2] = 6.0 + (double)((i * 5) % 8) * 0.5;
            // the projection under t = (0.53125, 0.0625 - 0.125 j, 0.03125) with an eighth of a pixel of pattern on top
            const double Z0 = c.Y[0] + 0.53125, Z1 = c.Y[1] + 0.0625 - 0.125 * (double)j, Z2 = c.Y[2] + 0.03125;
            c.u = Z0 / Z2 + ((double)(i % 3) - 1.0) / 6400.0, c.v = Z1 / Z2 + ((double)((i + 1) % 3) - 1.0) / 6400.0;
            c.b = i;
        }
    }
    const vslam::RefinedResection rs = vslam::refineResection(models, rows, cap, prm);
    hex("models", rs.models);
    hex("info", rs.info);
    hex("bits", rs.inlierBits);
    return 0;
}
