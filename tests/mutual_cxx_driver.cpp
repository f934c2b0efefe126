// Host driver of the C++ wrapper vslam::matchMutual (visualslam_amd/cxx/vslam_cxx.hpp), for tests/test_mutual_cpu.py and
// tests/test_gpu_mutual.py.  Without an argument it makes the calls that the wrapper refuses before it needs a GPU - a descriptor
// or a defined list of the wrong size - and prints "ok".  With --valid it makes one small valid call and prints "status N": 0 with
// a GPU, the ABI's VSLAM_ERR_HIP without one.
//   driver pair.bin RATIO out.bin
// pair.bin: two uint64 (query rows, train rows), the query descriptors, the train descriptors, the query defined bytes, the train
// defined bytes; out.bin: one uint64 and the nn records, one uint64 and the rnn records, one uint64 and the match records.
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
    const std::vector<std::vector<float>> two(2, std::vector<float>(128, 0.5f)), shortRow(2, std::vector<float>(127, 0.5f));
    if (argc < 2) {
        const std::vector<unsigned char> d3(3, 1);
        const bool ok = refused([&] { vslam::matchMutual(shortRow, two); }) && refused([&] { vslam::matchMutual(two, shortRow); }) &&
                        refused([&] { vslam::matchMutual(two, two, 0.8f, &d3); }) && refused([&] { vslam::matchMutual(two, two, 0.8f, nullptr, &d3); });
        std::printf(ok ? "ok\n" : "failed\n");
        return ok ? 0 : 1;
    }
    if (argc == 2 && std::strcmp(argv[1], "--valid") == 0) {
        int status = VSLAM_OK;
        try {
            const vslam::Matches r = vslam::matchMutual(two, two);
            if (r.nn.size() != 2 || r.rnn.size() != 2) status = 1;
        } catch (const vslam::Error& e) {
            status = e.status;
        }
        std::printf("status %d\n", status);
        return 0;
    }
    if (argc != 4) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t n[2];
    if (!get(f, n, 2)) return 2;
    std::vector<std::vector<float>> q(n[0], std::vector<float>(128)), t(n[1], std::vector<float>(128));
    std::vector<unsigned char> qd(n[0]), td(n[1]);
    for (auto& row : q)
        if (!get(f, row.data(), 128)) return 2;
    for (auto& row : t)
        if (!get(f, row.data(), 128)) return 2;
    if (!get(f, qd.data(), n[0]) || !get(f, td.data(), n[1])) return 2;
    std::fclose(f);
    try {
        const vslam::Matches r = vslam::matchMutual(q, t, std::strtof(argv[2], nullptr), &qd, &td);
        std::FILE* o = std::fopen(argv[3], "wb");
        if (!o) return 2;
        const uint64_t k[3] = {r.nn.size(), r.rnn.size(), r.matches.size()};
        std::fwrite(&k[0], sizeof k[0], 1, o);
        if (k[0]) std::fwrite(r.nn.data(), sizeof(vslam_nn2), k[0], o);
        std::fwrite(&k[1], sizeof k[1], 1, o);
        if (k[1]) std::fwrite(r.rnn.data(), sizeof(vslam_rnn), k[1], o);
        std::fwrite(&k[2], sizeof k[2], 1, o);
        if (k[2]) std::fwrite(r.matches.data(), sizeof(vslam_match), k[2], o);
        std::fclose(o);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "mutual_cxx_driver: %s\n", e.what());
        return 1;
    }
    return 0;
}
