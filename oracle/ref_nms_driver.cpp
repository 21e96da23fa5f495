// ---- compiled by oracle/ref_nms.mk against the reference's nms.hpp (TEST INFRASTRUCTURE ONLY) ----
//
// Runs the reference's own cv_dnn::NMSBoxes (nms.hpp of the reference tree: GetMaxScoreIndex with its std::stable_sort,
// NMSFast_'s walk with the adaptive threshold, jaccardDistance__ / rectOverlap) on box lists given in a file, so that
// tests can hold test_nms.py::py_nms, include/nms.hpp, csrc/sbm_nms_math.h and the device stage to what the reference
// computes.  The header is included from the reference tree; cv::Rect_ is the stand-in's (oracle/ref_cv), whose area()
// and operator& restate OpenCV's documented behaviour -- the one piece of the chain no binary here pins.
//
// usage: ref_nms INPUT OUTPUT
//   INPUT (little-endian): 'SBMN' magic (int32), n_problems (int32), then per problem
//     n (int32), score_threshold, nms_threshold, eta (f32), top_k (int32), n x (x, y, w, h int32, score f32)
//   OUTPUT: per problem n_kept (int32), then the kept indices (int32) in the order NMSBoxes returns them
//   One NMSBoxes call per problem.  A CV_Assert / CV_Error of the reference exits with status 3 and
//   "refused: <message>" on stderr.
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include <nms.hpp>

namespace sbm_ref_nms_driver {

struct Reader {
    FILE* f;
    int32_t i32() {
        int32_t v;
        if (std::fread(&v, 4, 1, f) != 1) throw std::runtime_error("truncated input");
        return v;
    }
    float f32() {
        float v;
        if (std::fread(&v, 4, 1, f) != 1) throw std::runtime_error("truncated input");
        return v;
    }
};

static int run(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s INPUT OUTPUT\n", argv[0]);
        return 2;
    }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) {
        std::fprintf(stderr, "cannot open %s\n", argv[2]);
        return 2;
    }
    Reader r{in};
    if (r.i32() != 0x4E4D4253) throw std::runtime_error("bad magic");
    const int n_problems = r.i32();
    if (n_problems < 0) throw std::runtime_error("bad header");
    for (int p = 0; p < n_problems; ++p) {
        const int n = r.i32();
        const float score_threshold = r.f32(), nms_threshold = r.f32(), eta = r.f32();
        const int top_k = r.i32();
        if (n < 0) throw std::runtime_error("bad problem size");
        std::vector<cv::Rect> boxes;
        std::vector<float> scores;
        boxes.reserve(n);
        scores.reserve(n);
        for (int i = 0; i < n; ++i) {
            const int x = r.i32(), y = r.i32(), w = r.i32(), h = r.i32();
            boxes.push_back(cv::Rect(x, y, w, h));
            scores.push_back(r.f32());
        }
        std::vector<int> kept;
        cv_dnn::NMSBoxes(boxes, scores, score_threshold, nms_threshold, kept, eta, top_k);
        const int32_t k = static_cast<int32_t>(kept.size());
        std::fwrite(&k, 4, 1, out);
        for (int v : kept) {
            const int32_t i = v;
            std::fwrite(&i, 4, 1, out);
        }
    }
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 2;
}

}  // namespace sbm_ref_nms_driver

int main(int argc, char** argv) {
    try {
        return sbm_ref_nms_driver::run(argc, argv);
    } catch (const cv::Exception& e) {
        std::fprintf(stderr, "refused: %s\n", e.what());
        return 3;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "driver error: %s\n", e.what());
        return 2;
    }
}
