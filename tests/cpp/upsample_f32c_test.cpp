// The C++ API's multi-channel f32 joint bilateral upsampling on files (tests/test_gpu_upsample_f32c_cpp.py):
//   upsample_f32c_test <dir> <width> <height> <scale> <ksize> <channels> <guide_channels>
// reads <dir>/src_lo.bin (float32, low_width x low_height x channels interleaved), guide_lo.bin and
// guide.bin (uint8), runs the dense blocking overload of CudaJointBilateralUpsample::upsample_f32c and
// writes <dir>/dst.bin (float32, width x height x channels). Plain C++ over include/cuda and the C
// ABI's buffer calls; no HIP header.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cuda/joint_bilateral_upsample.hpp"
#include "vip.h"

template <class T>
static std::vector<T> read_file(const std::string& path, size_t n) {
    std::vector<T> v(n);
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(v.data(), sizeof(T), n, f) != n) {
        std::fprintf(stderr, "cannot read %zu elements of %s\n", n, path.c_str());
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

static void write_file(const std::string& path, const std::vector<float>& v) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(float), v.size(), f) != v.size()) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        std::exit(2);
    }
    std::fclose(f);
}

static void check(int rc, const char* what) {
    if (rc) {
        std::fprintf(stderr, "%s: %s\n", what, vip_error_string(rc));
        std::exit(1);
    }
}

template <class T>
static T* to_device(const std::vector<T>& v) {
    void* d = nullptr;
    check(vip_malloc(&d, v.size() * sizeof(T)), "vip_malloc");
    check(vip_upload(d, v.data(), v.size() * sizeof(T)), "vip_upload");
    return static_cast<T*>(d);
}

int main(int argc, char** argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s dir width height scale ksize channels guide_channels\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), s = std::atoi(argv[4]), k = std::atoi(argv[5]),
              ch = std::atoi(argv[6]), gch = std::atoi(argv[7]);
    const CudaJointBilateralUpsample up(w, h, s, k);  // default sigmas: 1, 30
    const size_t n = (size_t)w * h, nlo = (size_t)up.low_width() * up.low_height();
    float* d_src = to_device(read_file<float>(dir + "/src_lo.bin", nlo * ch));
    std::uint8_t* d_guide_lo = to_device(read_file<std::uint8_t>(dir + "/guide_lo.bin", nlo * gch));
    std::uint8_t* d_guide = to_device(read_file<std::uint8_t>(dir + "/guide.bin", n * gch));
    float* d_dst = to_device(std::vector<float>(n * ch, -12345.f));

    up.upsample_f32c(d_src, ch, d_guide_lo, d_guide, gch, d_dst);  // blocking
    std::vector<float> out(n * ch);
    check(vip_download(out.data(), d_dst, out.size() * sizeof(float)), "vip_download");
    write_file(dir + "/dst.bin", out);

    for (void* p : {(void*)d_src, (void*)d_guide_lo, (void*)d_guide, (void*)d_dst}) check(vip_free(p), "vip_free");
    std::printf("upsample_f32c_test OK\n");
    return 0;
}
