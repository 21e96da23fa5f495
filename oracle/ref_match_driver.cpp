// ---- appended to the reference's line2Dup.cpp by oracle/ref_match.mk (TEST INFRASTRUCTURE ONLY) ----
//
// Runs the reference's own match half on quantized orientation maps given in a file, so that tests can compare the
// oracle and the HIP kernels with what the reference computes.  Appended to the same translation unit, this code can
// call the file-static spread / computeResponseMaps / linearize / similarity* / similarityLocal* and reaches the
// protected Detector::matchClass through a subclass.  Nothing of the gradient half runs.
//
// usage: ref_match_<variant> INPUT OUTPUT MODE [ARGS]
//   INPUT (little-endian int32 unless noted):
//     'SBMR' magic, n_levels, T[n_levels],
//     per level: rows, cols, rows*cols bytes of the quantized map (one-hot u8),
//     n_classes, per class: n_templates, per template, per level:
//       width, height, tl_x, tl_y, pyramid_level, n_features, then n_features x (x, y, label)
//   MODE and OUTPUT:
//     lm                    per level: T, W*H, then 8 x T*T x W*H bytes (spread -> computeResponseMaps -> linearize)
//     sim C I L             similarity map of template I of class C, level L (-1: the coarsest), dispatched on
//                           < 64 / < 8192 features as matchClass does: H, W, path (64 or 16), H*W u16
//     local L C I X Y       the 16 x 16 similarityLocal patch of that template at centre (X, Y): path, 256 u16
//     match THR             matchClass over every class (THR a float literal, hex allowed): the raw list, then the
//                           list after match()'s std::sort + std::unique; each as n, n x (x, y, f32 sim, class, id)
//   A CV_Assert / CV_Error of the reference exits with status 3 and "refused: <message>" on stderr.
namespace sbm_ref_driver {

using line2Dup::Detector;
using line2Dup::Feature;
using line2Dup::Match;
using line2Dup::Template;

struct Reader {
    FILE* f;
    int32_t i32() {
        int32_t v;
        if (std::fread(&v, 4, 1, f) != 1) throw std::runtime_error("truncated input");
        return v;
    }
};

struct Writer {
    FILE* f;
    void i32(int32_t v) { std::fwrite(&v, 4, 1, f); }
    void f32(float v) { std::fwrite(&v, 4, 1, f); }
    void bytes(const void* p, size_t n) { std::fwrite(p, 1, n, f); }
};

static std::string class_name(int c) { return cv::format("c%06d", c); }  // map order == class index order

class Harness : public Detector {
public:
    explicit Harness(std::vector<int> T) : Detector(T) {}

    std::vector<cv::Mat> quantized;
    LinearMemoryPyramid lm;
    std::vector<cv::Size> sizes;

    void add_class(int c, const std::vector<TemplatePyramid>& tps) { class_templates[class_name(c)] = tps; }
    const TemplatePyramid& pyramid(int c, int t) const { return class_templates.at(class_name(c)).at(t); }

    // Detector::match's linear-memory loop, fed with the given maps instead of the gradient stage's
    void build_linear_memories() {
        lm.assign(pyramid_levels, std::vector<LinearMemories>(1, LinearMemories(8)));
        sizes.clear();
        for (int l = 0; l < pyramid_levels; ++l) {
            int T = T_at_level[l];
            cv::Mat spread_quantized;
            std::vector<cv::Mat> response_maps;
            line2Dup::spread(quantized[l], spread_quantized, T);
            line2Dup::computeResponseMaps(spread_quantized, response_maps);
            for (int j = 0; j < 8; ++j) line2Dup::linearize(response_maps[j], lm[l][0][j], T);
            sizes.push_back(quantized[l].size());
        }
    }

    std::vector<Match> match_raw(float threshold) const {
        std::vector<Match> matches;
        for (TemplatesMap::const_iterator it = class_templates.begin(); it != class_templates.end(); ++it)
            matchClass(lm, sizes, threshold, matches, it->first, it->second);
        return matches;
    }
};

static int class_index(const std::string& name) { return std::atoi(name.c_str() + 1); }

static void write_matches(Writer& w, const std::vector<Match>& ms) {
    w.i32(static_cast<int32_t>(ms.size()));
    for (const Match& m : ms) {
        w.i32(m.x);
        w.i32(m.y);
        w.f32(m.similarity);
        w.i32(class_index(m.class_id));
        w.i32(m.template_id);
    }
}

static void write_u16(Writer& w, const cv::Mat& m) {
    CV_Assert(m.type() == CV_16U);
    for (int r = 0; r < m.rows; ++r) w.bytes(m.ptr(r), m.cols * 2);
}

static int run(int argc, char** argv) {
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s INPUT OUTPUT lm | sim C I L | local L C I X Y | match THR\n", argv[0]);
        return 2;
    }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) {
        std::fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    Reader r{in};
    if (r.i32() != 0x524D4253) throw std::runtime_error("bad magic");
    const int n_levels = r.i32();
    std::vector<int> T(n_levels);
    for (int& t : T) t = r.i32();
    Harness h(T);
    for (int l = 0; l < n_levels; ++l) {
        int rows = r.i32(), cols = r.i32();
        cv::Mat q(rows, cols, CV_8U);
        for (int y = 0; y < rows; ++y)
            if (std::fread(q.ptr(y), 1, cols, in) != size_t(cols)) throw std::runtime_error("truncated map");
        h.quantized.push_back(q);
    }
    const int n_classes = r.i32();
    for (int c = 0; c < n_classes; ++c) {
        std::vector<std::vector<Template>> tps(r.i32());
        for (auto& tp : tps) {
            tp.resize(n_levels);
            for (Template& t : tp) {
                t.width = r.i32();
                t.height = r.i32();
                t.tl_x = r.i32();
                t.tl_y = r.i32();
                t.pyramid_level = r.i32();
                t.features.resize(r.i32());
                for (Feature& f : t.features) {
                    f.x = r.i32();
                    f.y = r.i32();
                    f.label = r.i32();
                }
            }
        }
        h.add_class(c, tps);
    }
    std::fclose(in);

    const std::string mode = argv[3];
    h.build_linear_memories();
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) {
        std::fprintf(stderr, "cannot open %s\n", argv[2]);
        return 2;
    }
    Writer w{out};
    if (mode == "lm") {
        for (int l = 0; l < n_levels; ++l) {
            w.i32(T[l]);
            w.i32(h.lm[l][0][0].cols);
            for (int o = 0; o < 8; ++o) {
                const cv::Mat& m = h.lm[l][0][o];
                CV_Assert(m.rows == T[l] * T[l] && m.isContinuous());
                w.bytes(m.ptr(), m.total());
            }
        }
    } else if (mode == "sim" && argc == 7) {
        const auto& tp = h.pyramid(std::atoi(argv[4]), std::atoi(argv[5]));
        int l = std::atoi(argv[6]);
        if (l < 0) l = n_levels - 1;
        const Template& templ = tp[l];
        cv::Mat s;
        int path;
        if (templ.features.size() < 64) {
            line2Dup::similarity_64(h.lm[l][0], templ, s, h.sizes[l], T[l]);
            s.convertTo(s, CV_16U);
            path = 64;
        } else if (templ.features.size() < 8192) {
            line2Dup::similarity(h.lm[l][0], templ, s, h.sizes[l], T[l]);
            path = 16;
        } else {
            CV_Error(cv::Error::StsBadArg, "feature size too large");
        }
        w.i32(s.rows);
        w.i32(s.cols);
        w.i32(path);
        write_u16(w, s);
    } else if (mode == "local" && argc == 9) {
        const int l = std::atoi(argv[4]);
        const Template& templ = h.pyramid(std::atoi(argv[5]), std::atoi(argv[6]))[l];
        const cv::Point centre(std::atoi(argv[7]), std::atoi(argv[8]));
        cv::Mat s;
        int path;
        if (templ.features.size() < 64) {
            line2Dup::similarityLocal_64(h.lm[l][0], templ, s, h.sizes[l], T[l], centre);
            s.convertTo(s, CV_16U);
            path = 64;
        } else if (templ.features.size() < 8192) {
            line2Dup::similarityLocal(h.lm[l][0], templ, s, h.sizes[l], T[l], centre);
            path = 16;
        } else {
            CV_Error(cv::Error::StsBadArg, "feature size too large");
        }
        w.i32(path);
        write_u16(w, s);
    } else if (mode == "match" && argc == 5) {
        std::vector<Match> matches = h.match_raw(std::strtof(argv[4], nullptr));
        write_matches(w, matches);
        // Detector::match's epilogue
        std::sort(matches.begin(), matches.end());
        matches.erase(std::unique(matches.begin(), matches.end()), matches.end());
        write_matches(w, matches);
    } else {
        std::fprintf(stderr, "bad mode or arguments: %s\n", mode.c_str());
        std::fclose(out);
        return 2;
    }
    return std::fclose(out) == 0 ? 0 : 2;
}

}  // namespace sbm_ref_driver

int main(int argc, char** argv) {
    try {
        return sbm_ref_driver::run(argc, argv);
    } catch (const cv::Exception& e) {
        std::fprintf(stderr, "refused: %s\n", e.what());
        return 3;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "driver error: %s\n", e.what());
        return 2;
    }
}
