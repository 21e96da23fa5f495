// line2Dup_engine.h — the device side of line2Dup::Detector as the facade's translation units share it (line2Dup_amd.cpp:
// match, the batch entry points; line2Dup_verify.cpp: the verify stage): the pool of lanes, the lease of one, and the call
// that readies a lane's contexts.  Internal to the facade; include/line2Dup.h keeps Detector::Engine opaque.
#pragma once
#include "../../include/line2Dup.h"
#include "../../include/sbm.h"

#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace line2Dup {

// ---- device side: a pool of lanes -------------------------------------------------------------------------------
// The reference's match() is const and keeps no state (line2Dup.h:272-274): two threads may call it on one Detector.
// Here a call needs an engine context (device buffers sized for the frame, uploaded templates, a stream), which is not
// thread-safe.  So the Detector keeps a pool of LANES -- a lane = one context per device + what was uploaded / selected
// on them -- and every call takes a free lane for its duration: concurrent callers never share a context, a single
// caller only ever uses lane 0.  The vector of lanes grows under `mu` while other callers run, so it is only ever touched
// under `mu`; a caller works through the Lane* its lease took there (the lanes themselves never move).
struct Detector::Engine {
    struct Flat { // the TemplatesMap flattened for sbm_upload_templates, rebuilt when class_templates changed
        std::vector<sbm_template_level> levels;
        std::vector<sbm_feature> feats;
        std::vector<int32_t> cls, tid;
        std::vector<std::string> class_order; // class index -> id (map order = the order match() walks the classes, :1127-1129)
    };
    typedef std::map<std::string, cv::Mat> Fiducials; // Template::fiducial_src -> gray image (Detector::setFiducials)
    struct Lane {
        std::vector<sbm_ctx*> ctxs; // one per device
        std::shared_ptr<const Flat> uploaded;
        std::vector<int32_t> selected; // class selection currently active in the engine
        bool selection_valid = false;
        int selection_mode = 0; // 0: every context holds the whole selection; 1: sharded over the contexts
        int selection_rows = 0, selection_cols = 0; // geometry the shards were balanced for
        std::vector<unsigned char> recs; // match record scratch, kept between calls
        // the verify patches its contexts hold (line2Dup_verify.cpp): made from these fiducials for this upload of the templates
        std::shared_ptr<const Fiducials> verify_fiducials;
        std::shared_ptr<const Flat> verify_flat;
        bool busy = false;
    };
    // A batch of frames between begin() and end(): the one flow behind matchBatch, matchBatchNMS and matchAsync + wait.
    struct Batch {
        Lane* lane = nullptr;             // held by the caller's lease from before begin() until after end()
        std::shared_ptr<const Flat> flat; // null: nothing selected, nothing began, every list is empty
        // the frames (Mat headers: the pixels are the caller's and must stay unchanged until end()) and the mask(s) (a copy
        // when not continuous): the uploads begin() enqueues read them until end(), and a frame matched again needs them
        std::vector<cv::Mat> sources;
        cv::Mat mask8;
        std::vector<cv::Mat> masks8; // one per frame (the overloads that take a vector of masks), else empty
        float threshold = 0.f;
        int64_t cap = 1024;            // records per frame; the NMS-kept list is a subsequence of the raw list, so it fits too
        std::vector<int> first, count; // the frames of context d
        int begun = 0;                 // contexts [0, begun) began (those with count > 0) and must end

        void begin(const Detector& det, const std::vector<cv::Mat>& frames, float thr, const std::vector<std::string>& class_ids, const cv::Mat& mask,
                   const std::vector<cv::Mat>* masks);
        std::vector<std::vector<Match>> end(const Detector& det, const sbm_nms_params* nms, int bad = 0, std::string msg = std::string());
    };
    std::mutex mu;
    std::condition_variable cv;
    std::vector<std::unique_ptr<Lane>> lanes;
    int max_lanes = 4;
    std::shared_ptr<const Flat> flat; // null = class_templates changed since the last flattening
    std::shared_ptr<const Fiducials> fiducials; // Detector::setFiducials; null: none given
    std::map<const void*, std::pair<Lane*, sbm_ctx*>> pins; // pinBuffer: buffer -> (lane, context it is registered with)
    struct Async { // matchAsync ... wait: the detector's one batch in flight; batch.lane is set once it holds its lane
        bool active = false;
        Batch batch;
    } async;

    void templates_changed() // class_templates changed: the next call flattens and uploads again
    {
        std::lock_guard<std::mutex> lock(mu);
        flat.reset();
    }
    std::shared_ptr<const Flat> prepare(const Detector& det, Lane& lane, const std::vector<std::string>& class_ids, int rows, int cols, bool sharded);
    std::vector<std::vector<Match>> run_batch(const Detector& det, const std::vector<cv::Mat>& sources, float threshold,
                                              const std::vector<std::string>& class_ids, const cv::Mat& mask, const std::vector<cv::Mat>* masks,
                                              const sbm_nms_params* nms);
    void start_async(const Detector& det, const std::vector<cv::Mat>& sources, float threshold, const std::vector<std::string>& class_ids,
                     const cv::Mat& mask, const std::vector<cv::Mat>* masks);
};

namespace engine_detail {

typedef Detector::Engine Engine;

// take a free lane (want == null: any; else that one), creating an empty one while the pool may grow, else wait
inline Engine::Lane* acquire_lane(Engine& e, Engine::Lane* want = nullptr)
{
    std::unique_lock<std::mutex> lock(e.mu);
    for (;;) {
        if (want) {
            if (!want->busy) {
                want->busy = true;
                return want;
            }
        } else {
            for (auto& l : e.lanes)
                if (!l->busy) {
                    l->busy = true;
                    return l.get();
                }
            // a batch in flight (matchAsync ... wait) holds its lane between two calls of the SAME thread: it does not count
            // against the limit, or `matchAsync(); match(); wait();` with setConcurrency(1) would wait for itself
            if ((int)e.lanes.size() < e.max_lanes + (e.async.active && e.async.batch.lane ? 1 : 0)) {
                e.lanes.emplace_back(new Engine::Lane);
                e.lanes.back()->busy = true;
                return e.lanes.back().get();
            }
        }
        e.cv.wait(lock);
    }
}

struct LaneLease { // a lane taken under the pool's lock; released when the call ends, also by exception
    Engine* e;
    Engine::Lane* lane;
    ~LaneLease()
    {
        {
            std::lock_guard<std::mutex> lock(e->mu);
            lane->busy = false;
        }
        e->cv.notify_all();
    }
};

} // namespace engine_detail
} // namespace line2Dup
