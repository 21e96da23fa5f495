// ---- appended to the reference's line2Dup.cpp by oracle/ref_train.mk (TEST INFRASTRUCTURE ONLY) ----
//
// Runs the reference's own training half on gradient planes given in a file, so that tests can compare the oracle's
// add_template and the HIP training kernels with what the reference computes: ColorGradientPyramid::extractTemplate
// (with selectScatteredFeatures and the std::stable_sort) per level, then the file-static cropTemplates over the levels.
// Nothing of the gradient half runs: the magnitude, quantized-angle and angle_ori planes of every level, and the
// level's mask, are the caller's.
//
// How the ColorGradientPyramid is obtained.  Its members are public, but its constructor and pyrDown() call update().
// The object is constructed on an EMPTY source and an empty mask: on an empty Mat the stand-in's GaussianBlur, Sobel,
// phase, mul, +, convertTo and pyrDown return an empty Mat, so update() computes nothing (hysteresisGradient's loops
// run over zero rows).  Before extractTemplate, the level's planes and mask are stored into the object's members.
// Between the levels the reference's own pyrDown() runs on the (again empty) source and mask, so that num_features
// and pyramid_level change by the reference's statements and not by a restatement of them.
//
// usage: ref_train INPUT OUTPUT
//   INPUT (little-endian int32 unless noted):
//     'SBMT' magic, n_levels, num_features, strong_threshold (f32),
//     per level: rows, cols, has_mask, rows*cols f32 magnitude, rows*cols u8 quantized angle (one-hot),
//                rows*cols f32 angle_ori, and rows*cols u8 mask where has_mask != 0
//   OUTPUT:
//     failed_level (-1: every level succeeded), then, when it is -1, per level:
//       width, height, tl_x, tl_y, pyramid_level, n_features, then n_features x (x, y, label, f32 theta)
//   A CV_Assert / CV_Error of the reference exits with status 3 and "refused: <message>" on stderr.
namespace sbm_ref_train_driver {

using line2Dup::ColorGradientPyramid;
using line2Dup::Feature;
using line2Dup::Template;

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
    cv::Mat plane(int rows, int cols, int type) {
        cv::Mat m(rows, cols, type);
        const size_t row_bytes = size_t(cols) * m.elemSize();
        for (int y = 0; y < rows; ++y)
            if (std::fread(m.ptr(y), 1, row_bytes, f) != row_bytes) throw std::runtime_error("truncated plane");
        return m;
    }
};

struct Writer {
    FILE* f;
    void i32(int32_t v) { std::fwrite(&v, 4, 1, f); }
    void f32(float v) { std::fwrite(&v, 4, 1, f); }
};

struct Level {
    cv::Mat magnitude, angle, angle_ori, mask;
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
    Reader r{in};
    if (r.i32() != 0x544D4253) throw std::runtime_error("bad magic");
    const int n_levels = r.i32();
    const int num_features = r.i32();
    const float strong_threshold = r.f32();
    if (n_levels < 1 || num_features < 1) throw std::runtime_error("bad header");
    std::vector<Level> levels(n_levels);
    for (Level& lv : levels) {
        const int rows = r.i32(), cols = r.i32(), has_mask = r.i32();
        if (rows < 1 || cols < 1) throw std::runtime_error("bad level size");
        lv.magnitude = r.plane(rows, cols, CV_32F);
        lv.angle = r.plane(rows, cols, CV_8U);
        lv.angle_ori = r.plane(rows, cols, CV_32F);
        if (has_mask) lv.mask = r.plane(rows, cols, CV_8U);
    }
    std::fclose(in);

    // Detector::addTemplate's level loop (line2Dup.cpp:1317-1348) on a pyramid fed with the given planes instead of
    // the gradient stage's: pyrDown() before every level but the first, which halves num_features (:427) and counts
    // pyramid_level; the loop stops at the first level whose extractTemplate fails (:1342), where addTemplate returns
    // -1; cropTemplates runs over all levels once every one of them succeeded (:1348).
    std::vector<Template> tp(n_levels);
    ColorGradientPyramid qp(cv::Mat(), cv::Mat(), 0.0f, size_t(num_features), strong_threshold);
    int failed = -1;
    for (int l = 0; l < n_levels; ++l) {
        if (l > 0) {
            qp.magnitude = qp.angle = qp.angle_ori = qp.mask = cv::Mat();  // pyrDown() and update() see nothing
            qp.pyrDown();
        }
        CV_Assert(qp.pyramid_level == l && qp.src.empty());
        qp.magnitude = levels[l].magnitude;
        qp.angle = levels[l].angle;
        qp.angle_ori = levels[l].angle_ori;
        qp.mask = levels[l].mask;
        if (!qp.extractTemplate(tp[l])) {
            failed = l;
            break;
        }
    }
    if (failed < 0) line2Dup::cropTemplates(tp);

    FILE* out = std::fopen(argv[2], "wb");
    if (!out) {
        std::fprintf(stderr, "cannot open %s\n", argv[2]);
        return 2;
    }
    Writer w{out};
    w.i32(failed);
    if (failed < 0)
        for (const Template& t : tp) {
            w.i32(t.width);
            w.i32(t.height);
            w.i32(t.tl_x);
            w.i32(t.tl_y);
            w.i32(t.pyramid_level);
            w.i32(static_cast<int32_t>(t.features.size()));
            for (const Feature& f : t.features) {
                w.i32(f.x);
                w.i32(f.y);
                w.i32(f.label);
                w.f32(f.theta);
            }
        }
    return std::fclose(out) == 0 ? 0 : 2;
}

}  // namespace sbm_ref_train_driver

int main(int argc, char** argv) {
    try {
        return sbm_ref_train_driver::run(argc, argv);
    } catch (const cv::Exception& e) {
        std::fprintf(stderr, "refused: %s\n", e.what());
        return 3;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "driver error: %s\n", e.what());
        return 2;
    }
}
