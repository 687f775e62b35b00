// TEST INFRASTRUCTURE ONLY. A stand-in for the few OpenCV names the reference's include/cpp
// filters use as containers and as a loop driver, written here from scratch: dense row-major
// storage and a serial parallel_for_. It carries no arithmetic of any filter; the filters'
// own text is compiled from the reference where it lies (oracle/ref_cpp_filters.cpp).
// Not OpenCV, and not a substitute for it anywhere else.
#pragma once

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdlib>
#include <functional>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#define CV_OVERRIDE override
#define CV_32SC(n) (n)          // a type code here is the number of 4-byte channels
#define CV_32FC(n) (n)

namespace cv {

template <typename T, int N>
struct Vec {
    T val[N];
    Vec() : val{} {}
    Vec(T a, T b, T c) : val{a, b, c} { static_assert(N == 3, "three-element constructor"); }
    T& operator[](int i) { return val[i]; }
    const T& operator[](int i) const { return val[i]; }
};

template <typename T, int N>
Vec<T, N> operator+(const Vec<T, N>& a, const Vec<T, N>& b) {
    Vec<T, N> r;
    for (int i = 0; i < N; i++) r[i] = static_cast<T>(a[i] + b[i]);
    return r;
}

template <typename T, int N>
Vec<T, N> operator-(const Vec<T, N>& a, const Vec<T, N>& b) {
    Vec<T, N> r;
    for (int i = 0; i < N; i++) r[i] = static_cast<T>(a[i] - b[i]);
    return r;
}

using Vec3b = Vec<unsigned char, 3>;
using Vec3f = Vec<float, 3>;

struct Size {
    int width, height;
};

struct Scalar {
    double v;
    static Scalar all(double x) { return Scalar{x}; }
};

struct Range {
    int start, end;
    Range(int s, int e) : start(s), end(e) {}
};

struct ParallelLoopBody {
    virtual ~ParallelLoopBody() = default;
    virtual void operator()(const Range& range) const = 0;
};

inline void parallel_for_(const Range& range, const ParallelLoopBody& body) { body(range); }

// Typed dense 2-D array of V, row-major
template <typename V>
struct Mat_ {
    int rows = 0, cols = 0, dims = 2;
    std::vector<V> data;
    Mat_() = default;
    Mat_(int r, int c) : rows(r), cols(c), data(static_cast<std::size_t>(r) * c) {}
    void create(Size s) {
        rows = s.height;
        cols = s.width;
        data.assign(static_cast<std::size_t>(rows) * cols, V());
    }
    Size size() const { return Size{cols, rows}; }
    template <typename T>
    T& at(int y, int x) {
        static_assert(std::is_same_v<T, V>, "element type");
        return data[static_cast<std::size_t>(y) * cols + x];
    }
    template <typename T>
    const T& at(int y, int x) const {
        static_assert(std::is_same_v<T, V>, "element type");
        return data[static_cast<std::size_t>(y) * cols + x];
    }
    V& operator()(int y, int x) { return data[static_cast<std::size_t>(y) * cols + x]; }
    const V& operator()(int y, int x) const { return data[static_cast<std::size_t>(y) * cols + x]; }
};

using Mat3b = Mat_<Vec3b>;

// Untyped dense 2-D array of 4-byte channels (int or float, per the type code)
struct Mat {
    int rows = 0, cols = 0, channels = 0;
    std::vector<std::array<unsigned char, 4>> words;  // one 4-byte channel each, zero-initialised
    void create(int ndims, const int* sizes, int type) {
        (void)ndims;  // always 2: rows, cols
        rows = sizes[0];
        cols = sizes[1];
        channels = type;
        words.assign(static_cast<std::size_t>(rows) * cols * channels, {});
    }
    void setTo(const Scalar& s) {
        // only all-zero fills are supported: zero bytes are 0 and 0.0f alike
        if (s.v != 0.0) std::abort();
        std::fill(words.begin(), words.end(), std::array<unsigned char, 4>{});
    }
    template <typename T>
    T& at(int y, int x) {
        return *reinterpret_cast<T*>(words.data() + (static_cast<std::size_t>(y) * cols + x) * channels);
    }
    template <typename T>
    const T& at(int y, int x) const {
        return *reinterpret_cast<const T*>(words.data() + (static_cast<std::size_t>(y) * cols + x) * channels);
    }
};

}  // namespace cv
