// Stand-in for the part of OpenCV 4's core module that the reference's line2Dup.cpp compiles against.
//
// TEST INFRASTRUCTURE ONLY (oracle/ref_match.mk, oracle/ref_train.mk, oracle/ref_nms.mk).  Written for this project; it shares no code with OpenCV or with the
// product's own cv:: subset (include/sbm_cvlite.h), so that a misreading in one cannot hide on both sides of the
// comparison the reference binary makes.
//
// What the match half runs has a real body: Mat (create, zeros, ptr, at, step1, size, type, empty, ROI, clone,
// convertTo 8U -> 16U), Mat_, Size, Point, Rect, Ptr / makePtr, CV_Assert / CV_Error / Exception, format.
// The training half (oracle/ref_train.mk) adds what ColorGradientPyramid::extractTemplate itself calls: erode with the
// default 3x3 element and BORDER_REPLICATE, and the Mat(size, CV_8UC1, Scalar) fill.
// Everything else the file names (the gradient half's filters, FileStorage I/O, geometry transforms) is declared so
// the translation unit compiles, and throws cv::Exception if it is ever called on an image.  On an EMPTY Mat the
// gradient half's filters and Mat arithmetic (GaussianBlur, Sobel, phase, pyrDown, mul, +, convertTo) do nothing and
// return an empty Mat: that is how the training driver obtains a ColorGradientPyramid, whose constructor and pyrDown()
// call update(), without any gradient arithmetic (see oracle/ref_train_driver.cpp).
// The reference's nms.hpp (oracle/ref_nms.mk) uses Rect_::area() and operator&.  Both are restated here from OpenCV's
// documented behaviour (area = width * height; a & b = the intersection, or the empty Rect_() when the boxes share no
// extent in x or y).  With OpenCV absent, nothing checks this restatement against OpenCV's code: it is the one piece
// of the NMS oracle chain that stays unpinned.
//
// Allocation follows OpenCV: rows are continuous (step == cols * elemSize) and the buffer starts on a 64-byte
// boundary (orUnaligned8u's scalar prologue depends on the alignment).  Unlike OpenCV, every buffer is zero-filled and
// followed by a zeroed tail as long as the buffer itself, so reads past the last row (accessLinearMemory's overrun,
// similarityLocal's 16-row patch) see zeros instead of whatever the heap holds.
#ifndef SBM_REF_CV_CORE_HPP
#define SBM_REF_CV_CORE_HPP

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdlib.h>
#include <type_traits>
#include <iostream>
#include <limits>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

typedef unsigned char uchar;
typedef unsigned short ushort;

#define CV_8U 0
#define CV_8S 1
#define CV_16U 2
#define CV_16S 3
#define CV_32S 4
#define CV_32F 5
#define CV_64F 6
#define CV_CN_SHIFT 3
#define CV_MAT_DEPTH(t) ((t) & 7)
#define CV_MAT_CN(t) ((((t) >> CV_CN_SHIFT) & 63) + 1)
#define CV_MAKETYPE(depth, cn) (CV_MAT_DEPTH(depth) + (((cn) - 1) << CV_CN_SHIFT))
#define CV_8UC1 CV_MAKETYPE(CV_8U, 1)
#define CV_8UC3 CV_MAKETYPE(CV_8U, 3)
#define CV_16SC1 CV_MAKETYPE(CV_16S, 1)
#define CV_16SC3 CV_MAKETYPE(CV_16S, 3)
#define CV_32FC1 CV_MAKETYPE(CV_32F, 1)
#define CV_PI 3.1415926535897932384626433832795
#define CV_DECL_ALIGNED(x) __attribute__((aligned(x)))

namespace cv {

typedef std::string String;

namespace Error {
enum Code { StsOk = 0, StsError = -2, StsBadArg = -5, StsAssert = -215, StsNotImplemented = -213 };
}

class Exception : public std::runtime_error {
public:
    Exception(int c, const std::string& e, const std::string& f, const std::string& file, int l)
        : std::runtime_error(file + ":" + std::to_string(l) + ": " + (f.empty() ? "" : f + ": ") + e),
          code(c), err(e), func(f), line(l) {}
    int code;
    std::string err, func;
    int line;
};

inline String format(const char* fmt, ...) {
    va_list a, b;
    va_start(a, fmt);
    va_copy(b, a);
    int n = std::vsnprintf(nullptr, 0, fmt, a);
    va_end(a);
    std::vector<char> buf(n > 0 ? n + 1 : 1);
    std::vsnprintf(buf.data(), buf.size(), fmt, b);
    va_end(b);
    return String(buf.data());
}

[[noreturn]] inline void not_in_stand_in(const char* what) {
    throw Exception(Error::StsNotImplemented, std::string(what) + " is not part of the stand-in", what,
                    __FILE__, __LINE__);
}

}  // namespace cv

#define CV_Error(code, msg) throw ::cv::Exception((code), (msg), __func__, __FILE__, __LINE__)
#define CV_Assert(expr) \
    do { \
        if (!(expr)) throw ::cv::Exception(::cv::Error::StsAssert, #expr, __func__, __FILE__, __LINE__); \
    } while (0)
#define CV_DbgAssert(expr) ((void)0)

namespace cv {

template <typename T> struct Point_ {
    T x, y;
    Point_() : x(0), y(0) {}
    Point_(T x_, T y_) : x(x_), y(y_) {}
    Point_& operator/=(T s) { x /= s; y /= s; return *this; }
};
template <typename T> Point_<T> operator-(const Point_<T>& a, const Point_<T>& b) { return Point_<T>(a.x - b.x, a.y - b.y); }
template <typename T> Point_<T> operator+(const Point_<T>& a, const Point_<T>& b) { return Point_<T>(a.x + b.x, a.y + b.y); }
typedef Point_<int> Point;
typedef Point_<float> Point2f;

template <typename T> struct Size_ {
    T width, height;
    Size_() : width(0), height(0) {}
    Size_(T w, T h) : width(w), height(h) {}
    T area() const { return width * height; }
    bool operator==(const Size_& o) const { return width == o.width && height == o.height; }
    bool operator!=(const Size_& o) const { return !(*this == o); }
};
typedef Size_<int> Size;

template <typename T> struct Rect_ {
    T x, y, width, height;
    Rect_() : x(0), y(0), width(0), height(0) {}
    Rect_(T x_, T y_, T w, T h) : x(x_), y(y_), width(w), height(h) {}
    T area() const { return width * height; }
};
// the intersection: from the larger of the two origins to the smaller of the two far edges, per axis; the
// default-constructed empty rectangle when that leaves no extent in x or in y
template <typename T> Rect_<T> operator&(const Rect_<T>& a, const Rect_<T>& b) {
    const T x1 = std::max(a.x, b.x), y1 = std::max(a.y, b.y);
    const T x2 = std::min(a.x + a.width, b.x + b.width), y2 = std::min(a.y + a.height, b.y + b.height);
    if (x2 <= x1 || y2 <= y1) return Rect_<T>();
    return Rect_<T>(x1, y1, x2 - x1, y2 - y1);
}
typedef Rect_<int> Rect;

struct Scalar {
    double val[4];
    Scalar(double v0 = 0, double v1 = 0, double v2 = 0, double v3 = 0) : val{v0, v1, v2, v3} {}
};

template <typename T> using Ptr = std::shared_ptr<T>;
template <typename T, typename... A> Ptr<T> makePtr(A&&... a) { return std::make_shared<T>(std::forward<A>(a)...); }

enum BorderTypes { BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_DEFAULT = 4 };
enum InterpolationFlags { INTER_NEAREST = 0, INTER_LINEAR = 1 };
enum RotateFlags { ROTATE_90_CLOCKWISE = 0, ROTATE_180 = 1, ROTATE_90_COUNTERCLOCKWISE = 2 };

inline size_t elem_size1(int type) {
    static const size_t s[8] = {1, 1, 2, 2, 4, 4, 8, 0};
    return s[CV_MAT_DEPTH(type)];
}

class Mat {
public:
    int flags = 0;  // the type
    int rows = 0, cols = 0;
    size_t step = 0;  // bytes per row
    uchar* data = nullptr;
    std::shared_ptr<uchar> mem;

    Mat() {}
    Mat(int r, int c, int t) { create(r, c, t); }
    Mat(Size s, int t) { create(s.height, s.width, t); }
    Mat(int r, int c, int t, const Scalar& v) { create(r, c, t); setTo(v); }
    Mat(Size s, int t, const Scalar& v) { create(s.height, s.width, t); setTo(v); }
    Mat(const Mat& m, const Rect& roi) : Mat(m) {
        CV_Assert(roi.x >= 0 && roi.y >= 0 && roi.width >= 0 && roi.height >= 0 && roi.x + roi.width <= m.cols &&
                  roi.y + roi.height <= m.rows);
        data = m.data + roi.y * m.step + roi.x * elemSize();
        rows = roi.height;
        cols = roi.width;
    }

    void create(int r, int c, int t) {
        CV_Assert(r >= 0 && c >= 0 && CV_MAT_CN(t) >= 1);
        if (data && r == rows && c == cols && t == flags) return;
        flags = t;
        rows = r;
        cols = c;
        step = size_t(c) * elemSize();
        const size_t bytes = step * size_t(r);
        const size_t alloc = ((2 * bytes + 64 + 63) / 64) * 64;  // buffer + an equally long zero tail
        void* p = nullptr;
        if (posix_memalign(&p, 64, alloc) != 0) throw std::bad_alloc();
        std::memset(p, 0, alloc);
        mem = std::shared_ptr<uchar>(static_cast<uchar*>(p), [](uchar* q) { std::free(q); });
        data = mem.get();
    }
    void create(Size s, int t) { create(s.height, s.width, t); }

    static Mat zeros(int r, int c, int t) { return Mat(r, c, t); }
    static Mat zeros(Size s, int t) { return Mat(s, t); }

    int type() const { return flags; }
    int depth() const { return CV_MAT_DEPTH(flags); }
    int channels() const { return CV_MAT_CN(flags); }
    size_t elemSize() const { return elem_size1(flags) * channels(); }
    size_t elemSize1() const { return elem_size1(flags); }
    size_t step1() const { return step / elemSize1(); }
    size_t total() const { return size_t(rows) * cols; }
    bool empty() const { return data == nullptr || total() == 0; }
    bool isContinuous() const { return step == cols * elemSize() || rows == 1; }
    Size size() const { return Size(cols, rows); }

    uchar* ptr(int r = 0) { return data + size_t(r) * step; }
    const uchar* ptr(int r = 0) const { return data + size_t(r) * step; }
    template <typename T> T* ptr(int r = 0) { return reinterpret_cast<T*>(ptr(r)); }
    template <typename T> const T* ptr(int r = 0) const { return reinterpret_cast<const T*>(ptr(r)); }
    template <typename T> T& at(int r, int c) { return ptr<T>(r)[c]; }
    template <typename T> const T& at(int r, int c) const { return ptr<T>(r)[c]; }

    Mat operator()(const Rect& roi) const { return Mat(*this, roi); }

    Mat clone() const {
        Mat m(rows, cols, flags);
        for (int r = 0; r < rows; ++r) std::memcpy(m.ptr(r), ptr(r), cols * elemSize());
        return m;
    }
    void copyTo(Mat& dst) const {
        if (&dst != this) dst = clone();
    }
    void copyTo(Mat& dst, const Mat& mask) const;

    // the one conversion the match half makes: similarity_64's 8-bit sums widened to CV_16U, alpha 1, beta 0
    void convertTo(Mat& dst, int rtype, double alpha = 1, double beta = 0) const {
        if (empty()) {
            dst = Mat();
            return;
        }
        if (rtype < 0) rtype = depth();
        if (!(depth() == CV_8U && channels() == 1 && CV_MAT_DEPTH(rtype) == CV_16U && alpha == 1 && beta == 0))
            not_in_stand_in("Mat::convertTo (other than 8U -> 16U)");
        Mat out(rows, cols, CV_MAKETYPE(CV_16U, 1));
        for (int r = 0; r < rows; ++r) {
            const uchar* s = ptr(r);
            ushort* d = out.ptr<ushort>(r);
            for (int c = 0; c < cols; ++c) d[c] = s[c];
        }
        dst = out;
    }

    Mat& setTo(const Scalar& v) {
        if (depth() != CV_8U) not_in_stand_in("Mat::setTo (non-8U)");
        const int cn = channels();
        for (int r = 0; r < rows; ++r)
            for (int c = 0; c < cols; ++c)
                for (int k = 0; k < cn; ++k) ptr(r)[c * cn + k] = uchar(std::min(255.0, std::max(0.0, v.val[k & 3])));
        return *this;
    }

    Mat mul(const Mat& m, double = 1) const {
        if (empty() && m.empty()) return Mat();
        not_in_stand_in("Mat::mul");
    }
};

inline Mat operator+(const Mat& a, const Mat& b) {
    if (a.empty() && b.empty()) return Mat();
    not_in_stand_in("Mat + Mat");
}
inline Mat operator>(const Mat&, double) { not_in_stand_in("Mat > scalar"); }
inline void Mat::copyTo(Mat&, const Mat&) const { not_in_stand_in("Mat::copyTo with a mask"); }

template <typename T> class Mat_ : public Mat {
public:
    Mat_() {}
    Mat_(int r, int c) : Mat(r, c, type_of()) {}
    T& operator()(int r, int c) { return at<T>(r, c); }
    const T& operator()(int r, int c) const { return at<T>(r, c); }
    T* operator[](int r) { return ptr<T>(r); }
    const T* operator[](int r) const { return ptr<T>(r); }
    Mat_& operator=(const Mat& m) {
        Mat::operator=(m);
        return *this;
    }

private:
    static int type_of() {
        return std::is_same<T, uchar>::value ? CV_8U : std::is_same<T, ushort>::value ? CV_16U
             : std::is_same<T, short>::value ? CV_16S : std::is_same<T, float>::value ? CV_32F : CV_32S;
    }
};

// ---- the gradient half's filters: empty in, empty out; on an image they throw -----------------------------------
inline void empty_or_refuse(const Mat& src, Mat& dst, const char* what) {
    if (!src.empty()) not_in_stand_in(what);
    dst = Mat();
}
inline void GaussianBlur(const Mat& s, Mat& d, Size, double, double = 0, int = BORDER_DEFAULT) { empty_or_refuse(s, d, "GaussianBlur"); }
inline void Sobel(const Mat& s, Mat& d, int, int, int, int = 3, double = 1, double = 0, int = BORDER_DEFAULT) { empty_or_refuse(s, d, "Sobel"); }
inline void phase(const Mat& x, const Mat&, Mat& d, bool = false) { empty_or_refuse(x, d, "phase"); }
inline void pyrDown(const Mat& s, Mat& d, const Size& = Size(), int = BORDER_DEFAULT) { empty_or_refuse(s, d, "pyrDown"); }

// erode as extractTemplate calls it: the default element (an empty Mat: the 3x3 rectangle anchored at its centre), one
// iteration, BORDER_REPLICATE, on an 8-bit single-channel image -- the minimum over the window, rows and columns
// outside the image standing for the nearest one inside
inline void erode(const Mat& src, Mat& dst, const Mat& element, Point anchor = Point(-1, -1), int iterations = 1, int border = BORDER_CONSTANT) {
    if (!(element.empty() && anchor.x == -1 && anchor.y == -1 && iterations == 1 && border == BORDER_REPLICATE && src.type() == CV_8UC1 &&
          !src.empty()))
        not_in_stand_in("erode (other than 3x3, BORDER_REPLICATE, 8UC1)");
    Mat out(src.rows, src.cols, CV_8UC1);
    for (int r = 0; r < src.rows; ++r) {
        const uchar* up = src.ptr(std::max(r - 1, 0));
        const uchar* mid = src.ptr(r);
        const uchar* down = src.ptr(std::min(r + 1, src.rows - 1));
        for (int c = 0; c < src.cols; ++c) {
            const int left = std::max(c - 1, 0), right = std::min(c + 1, src.cols - 1);
            uchar m = std::min(std::min(up[left], up[c]), up[right]);
            m = std::min(m, std::min(std::min(mid[left], mid[c]), mid[right]));
            m = std::min(m, std::min(std::min(down[left], down[c]), down[right]));
            out.ptr(r)[c] = m;
        }
    }
    dst = out;
}
inline void resize(const Mat&, Mat&, Size, double = 0, double = 0, int = INTER_LINEAR) { not_in_stand_in("resize"); }
inline void rotate(const Mat&, Mat&, int) { not_in_stand_in("rotate"); }
inline void warpAffine(const Mat&, Mat&, const Mat&, Size, int = INTER_LINEAR, int = BORDER_CONSTANT, const Scalar& = Scalar()) { not_in_stand_in("warpAffine"); }
inline Mat getRotationMatrix2D(Point2f, double, double) { not_in_stand_in("getRotationMatrix2D"); }

class FileNode;
class FileNodeIterator {
public:
    FileNode operator*() const;
    FileNodeIterator& operator++() { not_in_stand_in("FileNodeIterator"); }
    bool operator!=(const FileNodeIterator&) const { not_in_stand_in("FileNodeIterator"); }
    template <typename T> FileNodeIterator& operator>>(T&) { not_in_stand_in("FileNodeIterator"); }
};

class FileNode {
public:
    FileNode operator[](const char*) const { not_in_stand_in("FileNode"); }
    FileNode operator[](const String&) const { not_in_stand_in("FileNode"); }
    FileNodeIterator begin() const { not_in_stand_in("FileNode"); }
    FileNodeIterator end() const { not_in_stand_in("FileNode"); }
    size_t size() const { not_in_stand_in("FileNode"); }
    operator int() const { not_in_stand_in("FileNode"); }
    operator float() const { not_in_stand_in("FileNode"); }
    operator double() const { not_in_stand_in("FileNode"); }
    operator String() const { not_in_stand_in("FileNode"); }
};
inline FileNode FileNodeIterator::operator*() const { not_in_stand_in("FileNodeIterator"); }
template <typename T> void operator>>(const FileNode&, T&) { not_in_stand_in("FileNode >>"); }

class FileStorage {
public:
    enum Mode { READ = 0, WRITE = 1 };
    FileStorage() {}
    FileStorage(const String&, int, const String& = String()) { not_in_stand_in("FileStorage"); }
    bool isOpened() const { return false; }
    void release() {}
    FileNode root() const { not_in_stand_in("FileStorage"); }
    FileNode operator[](const char*) const { not_in_stand_in("FileStorage"); }
    FileNode operator[](const String&) const { not_in_stand_in("FileStorage"); }
};
template <typename T> FileStorage& operator<<(FileStorage&, const T&) { not_in_stand_in("FileStorage <<"); }

}  // namespace cv

#endif
