// facade_driver.cpp -- runs the batch entry points of line2Dup::Detector (include/line2Dup.h, public API only) on the fake
// engine of fake_engine.cpp and prints, per scenario, what the calls returned and the engine calls they made
// (tests/test_facade_batch_paths.py).
//   facade_driver <templ_fmt> <class_id> all             every single-threaded scenario
//   facade_driver <templ_fmt> <class_id> threads <lanes>  8 threads x 200 calls on one detector with setConcurrency(lanes)
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/line2Dup.h"
#include "../../include/nms.hpp"
#include "fake_engine.h"

using namespace cv;
using line2Dup::Match;
typedef std::vector<Match> List;
typedef std::vector<List> Lists;

static std::string g_fmt, g_class;
static size_t g_printed = 0; // how much of the fake engine's log went out already
static const float THR = 80.f;
enum Entry { BATCH, ASYNC, NMS };
enum Masks { NONE, SHARED, SHARED_VIEW, VECTOR, EMPTY_VECTOR };
static const char* const ENTRY[] = {"matchBatch", "matchAsync+wait", "matchBatchNMS"};
static const char* const MASKS[] = {"no_mask", "shared_mask", "shared_mask_view", "mask_vector", "empty_mask_vector"};
struct Nms {
    float score, nms, eta;
    int top_k;
};
static const Nms KEEP_ALL = {-1.f, 1.f, 1.f, 0}, HALF = {0.f, 0.5f, 1.f, 0};

static bool same(const List& a, const List& b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (!(a[i] == b[i]) || a[i].template_id != b[i].template_id) return false;
    return true;
}

static bool same(const Lists& a, const Lists& b)
{
    if (a.size() != b.size()) return false;
    for (size_t f = 0; f < a.size(); ++f)
        if (!same(a[f], b[f])) return false;
    return true;
}

static void print_lists(const char* what, const Lists& l)
{
    uint32_t h = 2166136261u;
    printf("%s frames=%zu sizes=", what, l.size());
    for (size_t f = 0; f < l.size(); ++f) {
        printf("%s%zu", f ? "," : "", l[f].size());
        for (const Match& m : l[f]) {
            uint32_t v[4] = {(uint32_t)m.x, (uint32_t)m.y, 0, (uint32_t)m.template_id};
            memcpy(&v[2], &m.similarity, 4);
            for (size_t i = 0; i < sizeof v; ++i) h = (h ^ ((const unsigned char*)v)[i]) * 16777619u;
            for (char c : m.class_id) h = (h ^ (unsigned char)c) * 16777619u;
        }
    }
    printf(" hash=%08x\n", h);
}

static void print_throw(const char* what, const cv::Exception& e)
{
    // an assertion's text is its source expression: only the engine failures' texts are part of the contract
    if (e.code == Error::StsAssert) printf("%s throws StsAssert\n", what);
    else printf("%s throws %s text=[%s]\n", what, e.code == Error::StsBadArg ? "StsBadArg" : e.code == Error::StsError ? "StsError" : "other", e.err.c_str());
}

// the frames and masks of a scenario: frame f is F<f>, its own mask M<f>, the shared mask MS
struct Inputs {
    std::vector<Mat> frames, masks;
    Mat shared, wide;
    Inputs(int n, int rows, int cols, int type, Masks mode)
    {
        wide = Mat(rows, cols + 8, CV_8UC1, Scalar::all(0)); // the parent of the views that are not continuous
        for (int y = 0; y < rows; ++y)
            for (int x = 0; x < cols + 8; ++x) wide.ptr(y)[x] = (uchar)(x < 4 || y % 3 ? 200 + x : 0);
        for (int f = 0; f < n; ++f) {
            Mat m(rows, cols, type);
            const int rowbytes = cols * m.channels();
            for (int y = 0; y < rows; ++y)
                for (int x = 0; x < rowbytes; ++x) m.ptr(y)[x] = (uchar)(41 * f + 7 * x + 13 * y + 5);
            frames.push_back(m);
            fake_register(m.data, ("F" + std::to_string(f)).c_str());
        }
        if (mode == SHARED) {
            shared = Mat(rows, cols, CV_8UC1, Scalar::all(9));
            fake_register(shared.data, "MS");
        } else if (mode == SHARED_VIEW) {
            shared = wide(Rect(4, 0, cols, rows));
        } else if (mode == VECTOR) {
            for (int f = 0; f < n; ++f) {
                Mat m;
                if (f % 3 == 0) {
                    m = Mat(rows, cols, CV_8UC1, Scalar::all(17 + f));
                    fake_register(m.data, ("M" + std::to_string(f)).c_str());
                } else if (f % 3 == 2) {
                    m = wide(Rect(1 + f % 7, 0, cols, rows));
                } // f % 3 == 1: no mask for this frame
                masks.push_back(m);
            }
        }
    }
    const Mat& mask_of(size_t f) const { return masks.empty() ? shared : masks[f]; }
};

static void load(line2Dup::Detector& det, int contexts, int lanes)
{
    det.readClasses({g_class}, g_fmt);
    if (contexts > 1) det.setDevices(std::vector<int>((size_t)contexts, 0));
    if (lanes > 0) det.setConcurrency(lanes);
}

// what a loop of match() returns for the frames, on a detector of its own with one context; not logged, and its context
// is not counted
static Lists reference(const Inputs& in, const std::vector<std::string>& ids, const Nms* nms)
{
    fake_log_enable(false);
    Lists out;
    {
        line2Dup::Detector det(63, {4, 8});
        load(det, 1, 0);
        for (size_t f = 0; f < in.frames.size(); ++f) {
            const List all = det.match(in.frames[f], THR, ids, in.mask_of(f));
            if (!nms) {
                out.push_back(all);
                continue;
            }
            std::vector<Rect> boxes;
            std::vector<float> scores;
            for (const Match& m : all) {
                const auto& t = det.getTemplates(m.class_id, m.template_id);
                boxes.push_back(Rect(m.x, m.y, t[0].width, t[0].height));
                scores.push_back(m.similarity);
            }
            std::vector<int> idx;
            cv_dnn::NMSBoxes(boxes, scores, nms->score, nms->nms, idx, nms->eta, nms->top_k);
            List kept;
            for (int i : idx) kept.push_back(all[(size_t)i]);
            out.push_back(kept);
        }
    }
    fake_log_enable(true);
    return out;
}

static Lists call(const line2Dup::Detector& det, Entry e, const Inputs& in, Masks mode, const std::vector<std::string>& ids, const Nms& nms)
{
    const bool vec = mode == VECTOR || mode == EMPTY_VECTOR;
    if (e == BATCH) return vec ? det.matchBatch(in.frames, THR, ids, in.masks) : det.matchBatch(in.frames, THR, ids, in.shared);
    if (e == NMS)
        return vec ? det.matchBatchNMS(in.frames, THR, ids, nms.score, nms.nms, nms.eta, nms.top_k, in.masks)
                   : det.matchBatchNMS(in.frames, THR, ids, nms.score, nms.nms, nms.eta, nms.top_k, in.shared);
    if (vec) det.matchAsync(in.frames, THR, ids, in.masks);
    else det.matchAsync(in.frames, THR, ids, in.shared);
    return det.wait();
}

static void header(const char* kind, Entry e, Masks mode, int n, int rows, int cols, int type, int contexts)
{
    fake_reset();
    g_printed = 0;
    printf("== %s %s %s frames=%d %dx%dx%d contexts=%d\n", kind, ENTRY[e], MASKS[mode], n, rows, cols, type == CV_8UC1 ? 1 : 3, contexts);
}

// the engine calls logged since the last look
static void print_log()
{
    const std::string log = fake_log();
    printf("%s", log.c_str() + g_printed);
    g_printed = log.size();
}

// element f of every batch entry point equals match(frames[f], thr, ids, mask_f)
static void equal(Entry e, Masks mode, int n, int rows, int cols, int type, int contexts, bool all_classes, const Nms& nms = KEEP_ALL)
{
    header("equal", e, mode, n, rows, cols, type, contexts);
    const std::vector<std::string> ids = all_classes ? std::vector<std::string>() : std::vector<std::string>{g_class};
    const Inputs in(n, rows, cols, type, mode);
    Lists got;
    {
        line2Dup::Detector det(63, {4, 8});
        load(det, contexts, 0);
        got = call(det, e, in, mode, ids, nms);
    }
    const Lists want = reference(in, ids, e == NMS && nms.nms != 1.f ? &nms : nullptr);
    size_t total = 0;
    for (const List& l : want) total += l.size();
    printf("same=%d nonempty=%d\n", (int)same(got, want), (int)(total > 0));
    print_lists("lists", got);
    print_log();
}

static void unknown_class()
{
    fake_reset();
    g_printed = 0;
    printf("== unknown_class\n");
    const Inputs in(3, 16, 16, CV_8UC1, NONE);
    {
        line2Dup::Detector det(63, {4, 8});
        load(det, 2, 0);
        for (int e = 0; e < 3; ++e) {
            const Lists got = call(det, (Entry)e, in, e == 1 ? EMPTY_VECTOR : NONE, {"no_such_class"}, KEEP_ALL);
            int empty = got.size() == 3;
            for (const List& l : got) empty = empty && l.empty();
            printf("%s all_empty=%d\n", ENTRY[e], empty);
        }
    }
    print_log();
}

// frames whose list does not fit the batch's capacity are matched again alone, under their own mask, on context 0
static void capacity(Entry e)
{
    header("capacity", e, VECTOR, 6, 16, 16, CV_8UC3, 2);
    const Inputs in(6, 16, 16, CV_8UC3, VECTOR);
    fake_frame_reports(in.frames[1].data, 1500, false);  // more than the batch's 1024 per frame
    fake_frame_reports(in.frames[2].data, -1, false);    // a negative count
    fake_frame_reports(in.frames[3].data, INT_MIN, true); // the overflow word
    fake_frame_reports(in.frames[5].data, 5000, false);  // more than match_on_lane's first 4096
    Lists got;
    {
        line2Dup::Detector det(63, {4, 8});
        load(det, 2, 0);
        got = call(det, e, in, VECTOR, {g_class}, HALF);
    }
    const Lists want = reference(in, {g_class}, e == NMS ? &HALF : nullptr);
    printf("same=%d\n", (int)same(got, want));
    print_lists("lists", got);
    print_log();
}

// after a failure the lane and the async claim are free: with one lane, a batch and an async batch go through
static void recovery(const line2Dup::Detector& det, const Inputs& in, const Lists& want)
{
    printf("recovered_batch=%d\n", (int)same(det.matchBatch(in.frames, THR, {g_class}, in.masks), want));
    det.matchAsync(in.frames, THR, {g_class}, in.masks);
    printf("recovered_async=%d\n", (int)same(det.wait(), want));
}

static void failure(Entry e, bool in_begin, int code)
{
    const int contexts = in_begin ? 3 : 2, n = in_begin ? 5 : 3;
    header(in_begin ? "begin_fails" : "end_fails", e, VECTOR, n, 16, 16, CV_8UC1, contexts);
    const Inputs in(n, 16, 16, CV_8UC1, VECTOR);
    if (in_begin) fake_fail_begin(1, 0, code, "scripted: begin refused");
    else fake_fail_end(0, code, "scripted: end refused");
    const Lists want = reference(in, {g_class}, nullptr);
    {
        line2Dup::Detector det(63, {4, 8});
        load(det, contexts, 1);
        try {
            call(det, e, in, VECTOR, {g_class}, KEEP_ALL);
            printf("%s returned\n", ENTRY[e]);
        } catch (const cv::Exception& ex) {
            print_throw(ENTRY[e], ex);
        }
        print_log();
        printf("-- afterwards, on the one lane\n");
        recovery(det, in, want);
    }
    print_log();
}

static void async_rules()
{
    fake_reset();
    g_printed = 0;
    printf("== async_rules\n");
    const Inputs in(3, 32, 32, CV_8UC3, SHARED);
    const Lists want = reference(in, {g_class}, nullptr);
    {
        line2Dup::Detector det(63, {4, 8});
        load(det, 1, 1);
        try {
            det.wait();
            printf("wait with nothing in flight returned\n");
        } catch (const cv::Exception& ex) {
            print_throw("wait with nothing in flight", ex);
        }
        det.matchAsync(in.frames, THR, {g_class}, in.shared);
        printf("match between matchAsync and wait, one lane: same=%d\n", (int)same(det.match(in.frames[0], THR, {g_class}, in.shared), want[0]));
        try {
            det.matchAsync(in.frames, THR, {g_class}, in.shared);
            printf("second matchAsync returned\n");
        } catch (const cv::Exception& ex) {
            print_throw("second matchAsync", ex);
        }
        printf("wait same=%d\n", (int)same(det.wait(), want));
        try {
            det.matchAsync(std::vector<Mat>(), THR, {g_class});
            printf("matchAsync without frames returned\n");
        } catch (const cv::Exception& ex) {
            print_throw("matchAsync without frames", ex);
        }
        printf("matchBatch without frames: lists=%zu\n", det.matchBatch(std::vector<Mat>(), THR, {g_class}).size());
        printf("matchBatchNMS without frames: lists=%zu\n", det.matchBatchNMS(std::vector<Mat>(), THR, {g_class}, 0.f, 0.5f).size());
        const Inputs small(2, 16, 16, CV_8UC1, NONE);
        recovery(det, small, reference(small, {g_class}, nullptr));
    }
    print_log();
}

static void pins_and_growth()
{
    fake_reset();
    g_printed = 0;
    printf("== pins_and_growth\n");
    const Inputs in(2, 16, 16, CV_8UC1, NONE);
    fake_frame_reports(in.frames[1].data, 5000, false); // sbm_match: more than the first 4096
    const Lists want = reference(in, {g_class}, nullptr);
    {
        line2Dup::Detector det(63, {4, 8});
        load(det, 1, 0);
        det.pinBuffer(in.frames[0]);
        Lists got;
        for (const Mat& f : in.frames) got.push_back(det.match(f, THR, {g_class}));
        printf("same=%d\n", (int)same(got, want));
        print_lists("lists", got);
        det.unpinBuffer(in.frames[0]);
    }
    print_log();
}

// 8 threads x 200 calls on one detector, every fifth a matchBatch of 3 frames; every list equals the single caller's
static int threads(int lanes)
{
    fake_reset();
    fake_log_enable(false);
    const Inputs a(1, 16, 16, CV_8UC1, NONE), b(1, 32, 32, CV_8UC3, NONE);
    const std::vector<Mat> frames{a.frames[0], b.frames[0]};
    const std::vector<std::string> ids{g_class};
    line2Dup::Detector det(63, {4, 8});
    load(det, 1, lanes);
    Lists alone;
    for (const Mat& f : frames) alone.push_back(det.match(f, THR, ids));
    const int n_threads = 8, n_calls = 200;
    std::vector<int> bad((size_t)n_threads, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < n_threads; ++t)
        th.emplace_back([&, t]() {
            try {
                for (int i = 0; i < n_calls; ++i) {
                    const size_t k = (size_t)((t + i) & 1);
                    if (i % 5 == 4) {
                        for (const List& l : det.matchBatch({frames[k], frames[k], frames[k]}, THR, ids))
                            if (!same(l, alone[k])) ++bad[(size_t)t];
                    } else if (!same(det.match(frames[k], THR, ids), alone[k])) {
                        ++bad[(size_t)t];
                    }
                }
            } catch (const std::exception& e) {
                fprintf(stderr, "thread %d: %s\n", t, e.what());
                ++bad[(size_t)t];
            }
        });
    for (auto& t : th) t.join();
    int n_bad = 0;
    for (int v : bad) n_bad += v;
    printf("threads %d calls %d lanes %d matches %zu %zu different %d\n", n_threads, n_calls, lanes, alone[0].size(), alone[1].size(), n_bad);
    return n_bad ? 2 : 0;
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    g_fmt = argv[1];
    g_class = argv[2];
    try {
        if (std::string(argv[3]) == "threads") return threads(argc > 4 ? atoi(argv[4]) : 8);
        // 1, 2, 3 and 5 frames of 16 x 16 and 32 x 32, gray and BGR, over 1, 2 and 3 contexts; two frames over three
        // contexts and one frame over two leave a context without frames
        equal(BATCH, NONE, 1, 16, 16, CV_8UC1, 1, false);
        equal(BATCH, SHARED, 3, 32, 32, CV_8UC3, 2, true);
        equal(BATCH, VECTOR, 5, 16, 16, CV_8UC3, 3, false);
        equal(BATCH, EMPTY_VECTOR, 2, 32, 32, CV_8UC1, 3, false);
        equal(ASYNC, NONE, 2, 16, 16, CV_8UC3, 3, true);
        equal(ASYNC, SHARED_VIEW, 5, 32, 32, CV_8UC1, 2, false);
        equal(ASYNC, VECTOR, 3, 16, 16, CV_8UC1, 1, false);
        equal(ASYNC, EMPTY_VECTOR, 1, 32, 32, CV_8UC3, 2, false);
        equal(NMS, NONE, 3, 32, 32, CV_8UC3, 3, false);
        equal(NMS, SHARED, 2, 16, 16, CV_8UC1, 1, true);
        equal(NMS, VECTOR, 5, 32, 32, CV_8UC1, 2, false);
        equal(NMS, VECTOR, 3, 32, 32, CV_8UC3, 2, false, HALF);
        equal(NMS, EMPTY_VECTOR, 1, 16, 16, CV_8UC3, 1, false);
        unknown_class();
        for (int e = 0; e < 3; ++e) capacity((Entry)e);
        failure(BATCH, true, -1); // SBM_ERR_INVALID
        failure(ASYNC, true, -2); // SBM_ERR_HIP
        failure(NMS, true, -4);   // SBM_ERR_STATE
        failure(BATCH, false, -2);
        failure(ASYNC, false, -1);
        failure(NMS, false, -1);
        async_rules();
        pins_and_growth();
        return 0;
    } catch (const std::exception& e) {
        printf("driver: %s\n", e.what());
        return 1;
    }
}
