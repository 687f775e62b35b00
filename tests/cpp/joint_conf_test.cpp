// The C++ API's confidence-weighted f32 joint bilateral filter on files (tests/test_gpu_joint_conf_cpp.py):
//   joint_conf_test <dir> <width> <height> <ksize> <guide_channels> <hole_value>
// reads <dir>/src.bin, conf.bin (float32) and guide.bin (uint8), runs the dense blocking overload of
// CudaBilateralFilter::joint_bilateral_filter_conf_f32 with and without the weight output, and
// writes <dir>/dst.bin, weight.bin and dst_alone.bin (float32). Plain C++ over include/cuda and the
// C ABI's buffer calls; no HIP header.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cuda/bilateral_filter.hpp"
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

static std::vector<float> from_device(const float* d, size_t n) {
    std::vector<float> v(n);
    check(vip_download(v.data(), d, n * sizeof(float)), "vip_download");
    return v;
}

int main(int argc, char** argv) {
    if (argc != 7) {
        std::fprintf(stderr, "usage: %s dir width height ksize guide_channels hole_value\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), k = std::atoi(argv[4]), gch = std::atoi(argv[5]);
    const float hole = std::strtof(argv[6], nullptr);
    const size_t n = (size_t)w * h;
    float* d_src = to_device(read_file<float>(dir + "/src.bin", n));
    float* d_conf = to_device(read_file<float>(dir + "/conf.bin", n));
    std::uint8_t* d_guide = to_device(read_file<std::uint8_t>(dir + "/guide.bin", n * gch));
    const std::vector<float> fill(n, -12345.f);
    float* d_dst = to_device(fill);
    float* d_weight = to_device(fill);
    float* d_alone = to_device(fill);

    const CudaBilateralFilter filter(w, h, k);  // default sigmas: 10, 30
    filter.joint_bilateral_filter_conf_f32(d_src, d_conf, d_guide, gch, hole, d_dst, d_weight);  // blocking
    write_file(dir + "/dst.bin", from_device(d_dst, n));
    write_file(dir + "/weight.bin", from_device(d_weight, n));
    filter.joint_bilateral_filter_conf_f32(d_src, d_conf, d_guide, gch, hole, d_alone);  // d_weight = nullptr
    write_file(dir + "/dst_alone.bin", from_device(d_alone, n));

    for (void* p : {(void*)d_src, (void*)d_conf, (void*)d_guide, (void*)d_dst, (void*)d_weight, (void*)d_alone})
        check(vip_free(p), "vip_free");
    std::printf("joint_conf_test OK\n");
    return 0;
}
