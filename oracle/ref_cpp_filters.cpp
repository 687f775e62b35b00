// TEST INFRASTRUCTURE ONLY. Never built into, linked by or loaded from the product, and never
// shipped to the GPU box (oracle/_ref/ is untracked and stays on the development machine).
//
// The reference's include/cpp CPU filters -- bilateral_filter, joint_bilateral_filter
// (include/cpp/bilateral_filter.hpp) and adaptive_bilateral_filter
// (include/cpp/adaptive_bilateral_filter.hpp with border_replicated_integral_image.hpp) --
// compiled from the reference where they lie, whole and unmodified (oracle/Makefile gives
// -I$(REF)/include). They are the definition of the CPP numerics profile. Their
// <opencv2/core.hpp> resolves to oracle/cv_standin/opencv2/core.hpp, our own containers and a
// serial parallel_for_: the reference's arithmetic text is what runs, OpenCV's containers are
// not. tests/golden/make_ref_golden.py calls the entry points below and commits their outputs
// as tests/golden/ref_cpp_filters.npz.
//
// Same host build as ref_test_oracles.cpp: x86-64 without -march, -ffp-contract=off.
#include <cstdint>
#include <cstring>

#include "cpp/adaptive_bilateral_filter.hpp"
#include "cpp/bilateral_filter.hpp"

namespace {

cv::Mat3b load(const std::uint8_t* p, int width, int height) {
    cv::Mat3b m(height, width);
    std::memcpy(m.data.data(), p, static_cast<std::size_t>(width) * height * 3);
    return m;
}

void store(const cv::Mat3b& m, std::uint8_t* p) {
    std::memcpy(p, m.data.data(), m.data.size() * 3);
}

static_assert(sizeof(cv::Vec3b) == 3, "Vec3b is three packed bytes");

}  // namespace

extern "C" {

void ref_cpp_bilateral(const std::uint8_t* src, std::uint8_t* dst, int width, int height, int ksize,
                       float sigma_space, float sigma_color) {
    const cv::Mat3b s = load(src, width, height);
    cv::Mat3b d;
    bilateral_filter(s, d, ksize, sigma_space, sigma_color);
    store(d, dst);
}

void ref_cpp_joint(const std::uint8_t* src, const std::uint8_t* guide, std::uint8_t* dst, int width, int height,
                   int ksize, float sigma_space, float sigma_color) {
    const cv::Mat3b s = load(src, width, height), g = load(guide, width, height);
    cv::Mat3b d;
    joint_bilateral_filter(s, g, d, ksize, sigma_space, sigma_color);
    store(d, dst);
}

void ref_cpp_adaptive(const std::uint8_t* src, std::uint8_t* dst, int width, int height, int ksize,
                      float sigma_space, float sigma_color) {
    const cv::Mat3b s = load(src, width, height);
    cv::Mat3b d;
    adaptive_bilateral_filter(s, d, ksize, sigma_space, sigma_color);
    store(d, dst);
}

}  // extern "C"
