// fake_engine.cpp -- a stand-in for the 19 engine functions (include/sbm.h) that the Detector facade
// (shape_based_matching_amd/facade/line2Dup_amd.cpp, cvlite.cpp) links, for tests/test_facade_batch_paths.py: no GPU, no
// HIP.  It keeps the call rules of the real ones that the facade's batch path depends on (one batch in flight per context,
// _end ends it whatever it returns, SBM_ERR_CAPACITY with counts and overflow words, sbm_match's n_out > cap), logs every
// call, and fails where the driver's script says so.
//
// Match records are made up but deterministic: every ACTIVE template of the context decides from (the frame's first
// bytes, whether a mask was given and its first byte, the threshold, the template) whether it yields records and which,
// so a frame that travels with the wrong mask, threshold or selection gets another list, and the lists of template
// shards add up to the list of the whole selection.  Few distinct scores, exact duplicates and records that differ only in
// the template keep the epilogue (sbm_canonicalize, the facade's std::unique) busy.  sbm_canonicalize is the real one,
// restated; sbm_match_batch_host_end_nms applies the documented stage (epilogue, then include/nms.hpp's NMSBoxes).
#include "fake_engine.h"

#include <algorithm>
#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/nms.hpp"
#include "../../include/sbm.h"

namespace {

struct FrameScript {
    int n;
    bool overflow;
};
struct FailScript {
    int ctx, kth, code;
    std::string msg;
};
struct Global {
    std::mutex mu;
    int next_ctx = 0;
    bool log_on = true;
    std::string log;
    std::map<const void*, std::string> names;
    std::map<const void*, FrameScript> frames;
    std::vector<FailScript> begin_fails, end_fails;
} G;

thread_local std::string t_error;

int fail(int code, const std::string& msg)
{
    t_error = msg;
    return code;
}

uint32_t fnv(const void* p, size_t n, uint32_t h = 2166136261u)
{
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t*)p)[i]) * 16777619u;
    return h;
}

bool logging()
{
    std::lock_guard<std::mutex> lock(G.mu);
    return G.log_on;
}

void logf(const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    std::lock_guard<std::mutex> lock(G.mu);
    if (G.log_on) G.log += std::string(buf) + "\n";
}

std::string name_of(const void* p, size_t bytes)
{
    if (!p) return "-";
    {
        std::lock_guard<std::mutex> lock(G.mu);
        auto it = G.names.find(p);
        if (it != G.names.end()) return it->second;
    }
    char buf[32];
    snprintf(buf, sizeof buf, "copy:%08x", fnv(p, bytes));
    return buf;
}

uint32_t bits_of(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

} // namespace

struct sbm_ctx {
    int ord = 0, n_levels = 1, begins = 0;
    std::vector<int32_t> cls, tid, w0, h0; // per uploaded template
    std::vector<int32_t> active;           // selected template indices, in the order the engine walks them
    bool pending = false;                  // a batch between _begin and _end
    int64_t cap = 0;
    std::vector<std::vector<sbm_match_rec>> pend; // per frame of the pending batch: its stored records,
    std::vector<int32_t> pend_n, pend_over;       // the count it reports and its overflow word
};

namespace {

// the records of one frame on one context (see the head of the file); n_script >= 0: the list has exactly that many
std::vector<sbm_match_rec> frame_records(const sbm_ctx* c, const uint8_t* img, int rows, int cols, int channels, const uint8_t* mask,
                                         float threshold, int n_script)
{
    uint32_t key = fnv(img, (size_t)std::min(16, cols * channels));
    const uint8_t m[2] = {(uint8_t)(mask ? 1 : 0), (uint8_t)(mask ? mask[0] : 0)};
    key = fnv(m, 2, key);
    const uint32_t tb = bits_of(threshold);
    key = fnv(&tb, 4, key);
    std::vector<sbm_match_rec> out;
    const size_t nt = c->cls.size();
    for (int32_t t : c->active) {
        uint32_t h = fnv(&t, 4, key);
        h = (h ^ (h >> 15)) * 0x2c1b3c6du; // FNV's low bits only see the inputs' low bits
        h ^= h >> 13;
        if (h % 8) continue;
        sbm_match_rec r;
        r.x = (int32_t)((h >> 8) % (uint32_t)cols);
        r.y = (int32_t)((h >> 20) % (uint32_t)rows);
        r.raw = (int32_t)((h >> 5) % 8);
        r.similarity = 60.f + 5.f * (float)r.raw;
        r.class_idx = c->cls[(size_t)t];
        r.template_id = c->tid[(size_t)t];
        out.push_back(r);
        if ((h >> 3) % 4 == 0) out.push_back(r); // an exact duplicate
        if ((h >> 12) % 4 == 0) {                // the same place and score under the next template's label
            r.class_idx = c->cls[((size_t)t + 1) % nt];
            r.template_id = c->tid[((size_t)t + 1) % nt];
            out.push_back(r);
        }
    }
    if (n_script >= 0) {
        const size_t na = c->active.size();
        for (int i = (int)out.size(); i < n_script && na; ++i) {
            const int32_t t = c->active[(size_t)i % na];
            sbm_match_rec r;
            r.x = i % cols;
            r.y = (i / cols) % rows;
            r.raw = i;
            r.similarity = 40.f + (float)(i % 11);
            r.class_idx = c->cls[(size_t)t];
            r.template_id = c->tid[(size_t)t];
            out.push_back(r);
        }
        out.resize((size_t)n_script);
    }
    return out;
}

FrameScript script_of(const void* p)
{
    std::lock_guard<std::mutex> lock(G.mu);
    auto it = G.frames.find(p);
    return it == G.frames.end() ? FrameScript{INT_MIN, false} : it->second;
}

// the first scripted failure that matches, taken out of the script
bool take_fail(std::vector<FailScript>& v, int ctx, int kth, FailScript* out)
{
    std::lock_guard<std::mutex> lock(G.mu);
    for (size_t i = 0; i < v.size(); ++i)
        if (v[i].ctx == ctx && (v[i].kth < 0 || v[i].kth == kth)) {
            *out = v[i];
            v.erase(v.begin() + (long)i);
            return true;
        }
    return false;
}

int rec_cmp(const sbm_match_rec& x, const sbm_match_rec& y)
{
    if (x.similarity != y.similarity) return x.similarity > y.similarity ? -1 : 1;
    if (x.template_id != y.template_id) return x.template_id < y.template_id ? -1 : 1;
    if (x.class_idx != y.class_idx) return x.class_idx < y.class_idx ? -1 : 1;
    if (x.y != y.y) return x.y < y.y ? -1 : 1;
    if (x.x != y.x) return x.x < y.x ? -1 : 1;
    return 0;
}

int begin_batch(const char* what, sbm_ctx* c, const uint8_t* const* frames, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                int32_t channels, const uint8_t* shared_mask, const uint8_t* const* masks, float threshold, int64_t cap, int32_t sub_batch)
{
    int rc = 0;
    FailScript f;
    if (!frames || n_frames <= 0 || cap <= 0) rc = fail(SBM_ERR_INVALID, "bad batch arguments");
    else if (c->pending) rc = fail(SBM_ERR_STATE, "a batch is already in flight on this context");
    else if (take_fail(G.begin_fails, c->ord, c->begins, &f)) rc = fail(f.code, f.msg);
    ++c->begins;
    if (!rc) {
        c->pending = true;
        c->cap = cap;
        c->pend.clear();
        c->pend_n.clear();
        c->pend_over.clear();
        for (int32_t i = 0; i < n_frames; ++i) {
            const FrameScript s = script_of(frames[i]);
            const uint8_t* mask = masks ? masks[i] : shared_mask;
            std::vector<sbm_match_rec> r = frame_records(c, frames[i], rows, cols, channels, mask, threshold, s.n);
            c->pend_n.push_back(s.n != INT_MIN && s.n < 0 ? s.n : (int32_t)r.size());
            c->pend_over.push_back(s.overflow ? 1 : 0);
            if ((int64_t)r.size() > cap) r.resize((size_t)cap);
            c->pend.push_back(r);
        }
    }
    if (logging()) {
        std::string fr, mk;
        for (int32_t i = 0; frames && i < n_frames; ++i) {
            fr += (i ? "," : "") + name_of(frames[i], (size_t)rows * stride);
            if (masks) mk += (i ? "," : "") + name_of(masks[i], (size_t)rows * cols);
        }
        if (!masks) mk = name_of(shared_mask, (size_t)rows * cols);
        logf("%s ctx=%d n_frames=%d frames=%s %dx%dx%d step=%d %s=%s thr=%08x cap=%lld sub_batch=%d -> %d", what, c->ord, n_frames, fr.c_str(),
             rows, cols, channels, stride, masks ? "masks" : "mask", mk.c_str(), bits_of(threshold), (long long)cap, sub_batch, rc);
    }
    return rc;
}

// ends the pending batch; nms: the kept lists instead of the raw ones
int end_batch(const char* what, sbm_ctx* c, const sbm_nms_params* nms, sbm_match_rec* out, int64_t out_cap, int32_t* counts)
{
    int rc = 0;
    FailScript f;
    if (!c->pending) rc = fail(SBM_ERR_STATE, "no batch in flight on this context");
    else if (!out || !counts) rc = fail(SBM_ERR_INVALID, "null output");
    else if (take_fail(G.end_fails, c->ord, -1, &f)) rc = fail(f.code, f.msg);
    const size_t nf = c->pend.size();
    const bool was_pending = c->pending;
    c->pending = false; // _end ends the batch whatever it returns
    std::string cs;
    for (size_t i = 0; (!rc || rc == SBM_ERR_CAPACITY) && i < nf; ++i) {
        std::vector<sbm_match_rec> r = c->pend[i];
        int32_t n = c->pend_n[i], flags = c->pend_over[i];
        if (nms) {
            flags = (n < 0 || n > c->cap || flags) ? 1 : 0;
            r.resize((size_t)sbm_canonicalize(r.data(), (int64_t)r.size()));
            r.erase(std::unique(r.begin(), r.end(),
                                [](const sbm_match_rec& a, const sbm_match_rec& b) {
                                    return a.x == b.x && a.y == b.y && a.similarity == b.similarity && a.class_idx == b.class_idx;
                                }),
                    r.end());
            std::vector<cv::Rect> boxes;
            std::vector<float> scores;
            for (const sbm_match_rec& m : r) {
                int w = 0, h = 0;
                for (size_t t = 0; t < c->cls.size(); ++t)
                    if (c->cls[t] == m.class_idx && c->tid[t] == m.template_id) w = c->w0[t], h = c->h0[t];
                boxes.push_back(cv::Rect(m.x, m.y, w, h));
                scores.push_back(m.similarity);
            }
            std::vector<int> idx;
            cv_dnn::NMSBoxes(boxes, scores, nms->score_threshold, nms->nms_threshold, idx, nms->eta, nms->top_k);
            std::vector<sbm_match_rec> kept;
            for (int k : idx) kept.push_back(r[(size_t)k]);
            r = kept;
            n = (int32_t)r.size();
            if ((int64_t)n > out_cap) flags |= 2;
            if (flags & 3) rc = fail(SBM_ERR_CAPACITY, "a frame's list did not fit");
        } else if (n < 0 || n > c->cap || flags) {
            rc = fail(SBM_ERR_CAPACITY, "a frame's list did not fit");
        }
        const size_t stored = std::min(r.size(), (size_t)out_cap);
        if (stored) memcpy(out + i * (size_t)out_cap, r.data(), stored * sizeof(sbm_match_rec));
        counts[2 * i] = n;
        counts[2 * i + 1] = flags;
        cs += (i ? " " : "") + std::to_string(n) + "/" + std::to_string(flags);
    }
    if (nms)
        logf("%s ctx=%d pending=%d score=%08x nms=%08x eta=%08x top_k=%d out_cap=%lld -> %d counts=[%s]", what, c->ord, (int)was_pending,
             bits_of(nms->score_threshold), bits_of(nms->nms_threshold), bits_of(nms->eta), nms->top_k, (long long)out_cap, rc, cs.c_str());
    else
        logf("%s ctx=%d pending=%d -> %d counts=[%s]", what, c->ord, (int)was_pending, rc, cs.c_str());
    return rc;
}

int match_one(sbm_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t channels, const uint8_t* mask, float threshold,
              std::vector<sbm_match_rec>* all)
{
    if (!img || rows <= 0 || cols <= 0) return fail(SBM_ERR_INVALID, "bad frame");
    if (c->pending) return fail(SBM_ERR_STATE, "a batch is in flight on this context");
    const FrameScript s = script_of(img);
    const std::vector<sbm_match_rec> r = frame_records(c, img, rows, cols, channels, mask, threshold, s.n != INT_MIN && s.n >= 0 ? s.n : -1);
    all->insert(all->end(), r.begin(), r.end());
    return 0;
}

int deliver(const std::vector<sbm_match_rec>& all, sbm_match_rec* out, int64_t cap, int64_t* n_out)
{
    *n_out = (int64_t)all.size();
    const size_t stored = std::min(all.size(), (size_t)cap);
    if (stored) memcpy(out, all.data(), stored * sizeof(sbm_match_rec));
    return (int64_t)all.size() > cap ? fail(SBM_ERR_CAPACITY, "the list exceeds the output capacity") : 0;
}

} // namespace

void fake_reset()
{
    std::lock_guard<std::mutex> lock(G.mu);
    G.next_ctx = 0;
    G.log_on = true;
    G.log.clear();
    G.names.clear();
    G.frames.clear();
    G.begin_fails.clear();
    G.end_fails.clear();
}
void fake_register(const void* p, const char* name)
{
    std::lock_guard<std::mutex> lock(G.mu);
    G.names[p] = name;
}
void fake_log_enable(bool on)
{
    std::lock_guard<std::mutex> lock(G.mu);
    G.log_on = on;
}
std::string fake_log()
{
    std::lock_guard<std::mutex> lock(G.mu);
    return G.log;
}
void fake_fail_begin(int ctx, int kth, int code, const char* msg)
{
    std::lock_guard<std::mutex> lock(G.mu);
    G.begin_fails.push_back(FailScript{ctx, kth, code, msg});
}
void fake_fail_end(int ctx, int code, const char* msg)
{
    std::lock_guard<std::mutex> lock(G.mu);
    G.end_fails.push_back(FailScript{ctx, -1, code, msg});
}
void fake_frame_reports(const void* p, int n, bool overflow)
{
    std::lock_guard<std::mutex> lock(G.mu);
    G.frames[p] = FrameScript{n, overflow};
}

extern "C" {

const char* sbm_last_error(void) { return t_error.c_str(); }

int sbm_create(const sbm_config* cfg, sbm_ctx** out)
{
    sbm_ctx* c = new sbm_ctx;
    {
        std::lock_guard<std::mutex> lock(G.mu);
        c->ord = G.log_on ? G.next_ctx++ : -1; // contexts made while the log is off are not counted
    }
    c->n_levels = cfg->n_levels;
    *out = c;
    logf("sbm_create ctx=%d n_levels=%d T=%d,%d weak=%08x device=%d max_candidates=%lld -> 0", c->ord, cfg->n_levels, cfg->T[0], cfg->T[1],
         bits_of(cfg->weak_threshold), cfg->device_id, (long long)cfg->max_candidates);
    return 0;
}

void sbm_destroy(sbm_ctx* c)
{
    if (!c) return;
    logf("sbm_destroy ctx=%d pending=%d", c->ord, (int)c->pending);
    delete c;
}

int sbm_upload_templates(sbm_ctx* c, int32_t n, const sbm_template_level* levels, const sbm_feature* features, int64_t n_features,
                         const int32_t* class_idx, const int32_t* template_id)
{
    c->cls.assign(class_idx, class_idx + n);
    c->tid.assign(template_id, template_id + n);
    c->w0.clear();
    c->h0.clear();
    for (int32_t t = 0; t < n; ++t) {
        c->w0.push_back(levels[(size_t)t * c->n_levels].width);
        c->h0.push_back(levels[(size_t)t * c->n_levels].height);
    }
    c->active.resize((size_t)n);
    for (int32_t t = 0; t < n; ++t) c->active[(size_t)t] = t;
    logf("sbm_upload_templates ctx=%d n_templates=%d n_features=%lld features=%08x -> 0", c->ord, n, (long long)n_features,
         fnv(features, (size_t)n_features * sizeof(sbm_feature)));
    return 0;
}

int sbm_select_classes(sbm_ctx* c, const int32_t* class_idx, int32_t n)
{
    c->active.clear();
    std::string s;
    if (n == 0)
        for (size_t t = 0; t < c->cls.size(); ++t) c->active.push_back((int32_t)t);
    for (int32_t i = 0; i < n; ++i) {
        s += (i ? "," : "") + std::to_string(class_idx[i]);
        for (size_t t = 0; t < c->cls.size(); ++t)
            if (c->cls[t] == class_idx[i]) c->active.push_back((int32_t)t);
    }
    logf("sbm_select_classes ctx=%d classes=[%s] -> 0 active=%zu", c->ord, s.c_str(), c->active.size());
    return 0;
}

int sbm_select_templates(sbm_ctx* c, const int32_t* template_idx, int32_t n)
{
    c->active.assign(template_idx, template_idx + n);
    logf("sbm_select_templates ctx=%d n=%d first=%d list=%08x -> 0", c->ord, n, n ? template_idx[0] : -1, fnv(template_idx, (size_t)n * 4));
    return 0;
}

int sbm_partition_templates(sbm_ctx* c, int32_t rows, int32_t cols, const int32_t* template_idx, int32_t n, int32_t n_shards, int32_t* first,
                            int32_t* count)
{
    (void)template_idx;
    for (int32_t s = 0; s < n_shards; ++s) {
        first[s] = (int32_t)((int64_t)n * s / n_shards);
        count[s] = (int32_t)((int64_t)n * (s + 1) / n_shards) - first[s];
    }
    logf("sbm_partition_templates ctx=%d %dx%d n=%d n_shards=%d -> 0", c->ord, rows, cols, n, n_shards);
    return 0;
}

int sbm_match(sbm_ctx* c, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride, int32_t channels, const uint8_t* mask, float threshold,
              sbm_match_rec* out, int64_t cap, int64_t* n_out)
{
    std::vector<sbm_match_rec> all;
    int rc = match_one(c, img, rows, cols, channels, mask, threshold, &all);
    if (!rc) rc = deliver(all, out, cap, n_out);
    if (logging())
        logf("sbm_match ctx=%d frame=%s %dx%dx%d step=%d mask=%s thr=%08x cap=%lld -> %d n=%lld", c->ord, name_of(img, (size_t)rows * stride).c_str(),
             rows, cols, channels, stride, name_of(mask, (size_t)rows * cols).c_str(), bits_of(threshold), (long long)cap, rc, (long long)all.size());
    return rc;
}

int sbm_match_sharded(sbm_ctx* const* ctxs, int32_t n_ctx, const uint8_t* img, int32_t rows, int32_t cols, int32_t stride, int32_t channels,
                      const uint8_t* mask, float threshold, sbm_match_rec* out, int64_t cap, int64_t* n_out)
{
    std::vector<sbm_match_rec> all;
    int rc = 0;
    std::string cs;
    for (int32_t i = 0; i < n_ctx; ++i) {
        cs += (i ? "," : "") + std::to_string(ctxs[i]->ord);
        if (!rc) rc = match_one(ctxs[i], img, rows, cols, channels, mask, threshold, &all);
    }
    if (!rc) rc = deliver(all, out, cap, n_out);
    if (logging())
        logf("sbm_match_sharded ctxs=%s frame=%s %dx%dx%d step=%d mask=%s thr=%08x cap=%lld -> %d n=%lld", cs.c_str(),
             name_of(img, (size_t)rows * stride).c_str(), rows, cols, channels, stride, name_of(mask, (size_t)rows * cols).c_str(), bits_of(threshold),
             (long long)cap, rc, (long long)all.size());
    return rc;
}

int sbm_match_batch_host_begin(sbm_ctx* c, const uint8_t* const* frames, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                               int32_t channels, const uint8_t* mask, float threshold, int64_t cap, int32_t sub_batch)
{
    return begin_batch("sbm_match_batch_host_begin", c, frames, n_frames, rows, cols, stride, channels, mask, nullptr, threshold, cap, sub_batch);
}

int sbm_match_batch_host_begin_masked(sbm_ctx* c, const uint8_t* const* frames, int32_t n_frames, int32_t rows, int32_t cols, int32_t stride,
                                      int32_t channels, const uint8_t* const* masks, float threshold, int64_t cap, int32_t sub_batch)
{
    if (!masks) return fail(SBM_ERR_INVALID, "null mask list");
    return begin_batch("sbm_match_batch_host_begin_masked", c, frames, n_frames, rows, cols, stride, channels, nullptr, masks, threshold, cap,
                       sub_batch);
}

int sbm_match_batch_host_end(sbm_ctx* c, sbm_match_rec* out, int32_t* counts)
{
    return end_batch("sbm_match_batch_host_end", c, nullptr, out, c->cap, counts);
}

int sbm_match_batch_host_end_nms(sbm_ctx* c, const sbm_nms_params* p, sbm_match_rec* out, int64_t out_cap, int32_t* counts)
{
    if (!p) return fail(SBM_ERR_INVALID, "null parameters");
    return end_batch("sbm_match_batch_host_end_nms", c, p, out, out_cap, counts);
}

int sbm_pin_host_buffer(sbm_ctx* c, const void* p, int64_t bytes)
{
    logf("sbm_pin_host_buffer ctx=%d buffer=%s bytes=%lld -> 0", c->ord, name_of(p, 0).c_str(), (long long)bytes);
    return 0;
}

int sbm_unpin_host_buffer(sbm_ctx* c, const void* p)
{
    logf("sbm_unpin_host_buffer ctx=%d buffer=%s -> 0", c->ord, name_of(p, 0).c_str());
    return 0;
}

// the real one (csrc/sbm_capi_match.inc), restated; pure, so not logged
int64_t sbm_canonicalize(sbm_match_rec* recs, int64_t n)
{
    if (!recs || n <= 0) return 0;
    std::sort(recs, recs + n, [](const sbm_match_rec& a, const sbm_match_rec& b) { return rec_cmp(a, b) < 0; });
    int64_t k = 1;
    for (int64_t i = 1; i < n; ++i)
        if (rec_cmp(recs[i], recs[k - 1]) != 0) recs[k++] = recs[i];
    return k;
}

// the training side is not what this stand-in is for
int sbm_quantized_orientations(sbm_ctx*, const uint8_t*, int32_t, int32_t, int32_t, int32_t, float, float*, uint8_t*, float*)
{
    return fail(SBM_ERR_STATE, "not in the fake engine");
}
int sbm_pyrdown(sbm_ctx*, const uint8_t*, int32_t, int32_t, int32_t, int32_t, uint8_t*) { return fail(SBM_ERR_STATE, "not in the fake engine"); }
int sbm_extract_local_maxima(sbm_ctx*, const float*, const uint8_t*, int32_t, int32_t, float, int32_t*, int64_t, int64_t*)
{
    return fail(SBM_ERR_STATE, "not in the fake engine");
}

} // extern "C"
