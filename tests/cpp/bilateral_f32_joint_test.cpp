// The C++ API's f32 joint bilateral filter under an f32 guide on files
// (tests/test_gpu_bilateral_f32_joint_cpp.py):
//   bilateral_f32_joint_test <dir> <width> <height> <ksize> <sigma_space> <sigma_color> <value_range>
// reads <dir>/src.bin and guide.bin (float32), runs the dense blocking overload of
// CudaBilateralFilterF32::joint_bilateral_filter, the stream overload on the default stream followed
// by a device synchronisation, and the C ABI's vip_bilateral_f32_run_joint on a handle of its own,
// and writes <dir>/dst.bin, dst_stream.bin and dst_capi.bin (float32). Plain C++ over include/cuda
// and the C ABI's buffer calls; no HIP header.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "cuda/bilateral_filter_f32.hpp"
#include "vip.h"

static std::vector<float> read_file(const std::string& path, size_t n) {
    std::vector<float> v(n);
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(v.data(), sizeof(float), n, f) != n) {
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

static float* to_device(const std::vector<float>& v) {
    void* d = nullptr;
    check(vip_malloc(&d, v.size() * sizeof(float)), "vip_malloc");
    check(vip_upload(d, v.data(), v.size() * sizeof(float)), "vip_upload");
    return static_cast<float*>(d);
}

static std::vector<float> from_device(const float* d, size_t n) {
    std::vector<float> v(n);
    check(vip_download(v.data(), d, n * sizeof(float)), "vip_download");
    return v;
}

int main(int argc, char** argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s dir width height ksize sigma_space sigma_color value_range\n", argv[0]);
        return 2;
    }
    const std::string dir = argv[1];
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]), k = std::atoi(argv[4]);
    const float ss = std::strtof(argv[5], nullptr), sc = std::strtof(argv[6], nullptr);
    const float range = std::strtof(argv[7], nullptr);
    const size_t n = (size_t)w * h;
    float* d_src = to_device(read_file(dir + "/src.bin", n));
    float* d_guide = to_device(read_file(dir + "/guide.bin", n));
    const std::vector<float> fill(n, -12345.f);
    float* d_dst = to_device(fill);
    float* d_stream = to_device(fill);
    float* d_capi = to_device(fill);

    const CudaBilateralFilterF32 filter(w, h, k, ss, sc, range);
    filter.joint_bilateral_filter(d_src, d_guide, d_dst);  // blocking
    write_file(dir + "/dst.bin", from_device(d_dst, n));
    filter.joint_bilateral_filter(d_src, d_guide, d_stream, nullptr);  // enqueues on the default stream
    check(vip_device_synchronize(), "vip_device_synchronize");
    write_file(dir + "/dst_stream.bin", from_device(d_stream, n));

    vip_bilateral_f32_t handle = nullptr;
    check(vip_bilateral_f32_create(&handle, w, h, k, ss, sc, range, VIP_NUMERICS_CUDA), "vip_bilateral_f32_create");
    const size_t pitch = (size_t)w * sizeof(float);
    check(vip_bilateral_f32_run_joint(handle, d_src, pitch, d_guide, pitch, d_capi, pitch, nullptr),
          "vip_bilateral_f32_run_joint");
    check(vip_device_synchronize(), "vip_device_synchronize");
    write_file(dir + "/dst_capi.bin", from_device(d_capi, n));
    check(vip_bilateral_f32_destroy(handle), "vip_bilateral_f32_destroy");

    for (void* p : {(void*)d_src, (void*)d_guide, (void*)d_dst, (void*)d_stream, (void*)d_capi})
        check(vip_free(p), "vip_free");
    std::printf("bilateral_f32_joint_test OK\n");
    return 0;
}
