// line2Dup_verify.cpp — the verify stage of line2Dup::Detector: what the reference's production driver does with the matches
// NMS kept (HCORR, test_jabil.cpp:152-207).  Detector::verifyPatch makes a template's fiducial patch as the driver does
// (test_jabil.cpp:187-191, utils.cpp:157-187), setFiducials takes the driver's map of fiducial images (utils.cpp:236-243) and
// matchBatchVerified runs match, NMS and the correlation filter on the device through sbm_match_batch_host_verified.  The
// pixels' arithmetic is the engine's (include/sbm.h, "verify rule"); this file only makes patches and moves lists.
#include "line2Dup_engine.h"
#include "line2Dup_verify_patch.h"

#include <algorithm>

using namespace cv;

namespace line2Dup {

namespace {

typedef Detector::Engine Engine;
using engine_detail::acquire_lane;
using engine_detail::LaneLease;

void check(int rc, const char* what)
{
    if (rc != 0) CV_Error(rc == SBM_ERR_INVALID ? Error::StsBadArg : Error::StsError, std::string(what) + ": " + sbm_last_error());
}

} // namespace

Mat Detector::verifyPatch(const Template& t0, const Mat& fiducial_gray) { return verify_patch_of(t0, fiducial_gray); }

void Detector::setFiducials(const std::map<std::string, Mat>& gray_by_src)
{
    std::shared_ptr<Engine::Fiducials> f(new Engine::Fiducials);
    for (const auto& kv : gray_by_src) {
        CV_Assert(kv.second.empty() || kv.second.type() == CV_8UC1);
        (*f)[kv.first] = kv.second.clone(); // the caller's images may change after the call
    }
    std::lock_guard<std::mutex> lock(eng_->mu);
    eng_->fiducials = f; // every lane's contexts take the new patches when next used
}

std::vector<std::vector<Detector::VerifiedMatch>> Detector::matchBatchVerified(const std::vector<Mat>& sources, float threshold,
                                                                                const std::vector<std::string>& class_ids, float score_threshold,
                                                                                float nms_threshold, double min_corr, float eta, int top_k,
                                                                                bool keep_unverified) const
{
    std::vector<std::vector<VerifiedMatch>> out(sources.size());
    if (sources.empty()) return out;
    const Mat& s0 = sources[0];
    for (const Mat& s : sources)
        CV_Assert(!s.empty() && (s.type() == CV_8UC1 || s.type() == CV_8UC3) && s.type() == s0.type() && s.size() == s0.size() && s.step == s0.step);
    Engine& e = *eng_;
    LaneLease lease{&e, acquire_lane(e)};
    Engine::Lane& lane = *lease.lane;
    const std::shared_ptr<const Engine::Flat> flat = e.prepare(*this, lane, class_ids, s0.rows, s0.cols, false);
    if (!flat) return out;
    // the patches of this upload of the templates, on every context of the lane: made once per change of either
    std::shared_ptr<const Engine::Fiducials> fids;
    {
        std::lock_guard<std::mutex> lock(e.mu);
        fids = e.fiducials;
    }
    if (lane.verify_flat != flat || lane.verify_fiducials != fids) {
        std::vector<Mat> patches; // (keeps the pixels alive until the uploads are done)
        std::vector<sbm_verify_patch> recs;
        int ci = 0;
        for (const auto& kv : class_templates) { // the order Engine::prepare numbers the classes in
            for (size_t t = 0; t < kv.second.size() && fids; ++t) {
                const Template& t0 = kv.second[t][0];
                const auto it = fids->find(t0.fiducial_src);
                if (it == fids->end()) continue;
                const Mat p = verifyPatch(t0, it->second);
                if (p.empty()) continue;
                patches.push_back(p);
                recs.push_back(sbm_verify_patch{ci, (int32_t)t, p.cols, p.rows, (int32_t)p.step, 0, p.data});
            }
            ++ci;
        }
        for (sbm_ctx* c : lane.ctxs) check(sbm_upload_verify_patches(c, recs.empty() ? nullptr : recs.data(), (int32_t)recs.size()), "sbm_upload_verify_patches");
        lane.verify_flat = flat;
        lane.verify_fiducials = fids;
    }
    const sbm_nms_params nms{score_threshold, nms_threshold, eta, top_k};
    const sbm_verify_params vp{min_corr, keep_unverified ? 1 : 0, 0};
    // the frames dealt over the lane's contexts in contiguous groups, as matchBatch deals them
    const int D = (int)lane.ctxs.size(), n = (int)sources.size();
    for (int d = 0; d < D; ++d) {
        const int first = (int)((int64_t)n * d / D), count = (int)((int64_t)n * (d + 1) / D) - first;
        if (!count) continue;
        std::vector<const uint8_t*> ptrs((size_t)count);
        for (int f = 0; f < count; ++f) ptrs[(size_t)f] = sources[(size_t)(first + f)].data;
        // a raw list or a kept list that does not fit (SBM_ERR_CAPACITY): again with four times the room
        for (int64_t cap = 1024;; cap *= 4) {
            std::vector<sbm_match_rec> recs((size_t)count * cap);
            std::vector<float> scores((size_t)count * cap);
            std::vector<int32_t> cnt((size_t)count * 2);
            const int rc = sbm_match_batch_host_verified(lane.ctxs[(size_t)d], ptrs.data(), count, s0.rows, s0.cols, (int32_t)s0.step, s0.channels(), threshold,
                                                         cap, &nms, &vp, recs.data(), scores.data(), cap, cnt.data());
            if (rc == SBM_ERR_CAPACITY && cap < ((int64_t)1 << 22)) continue;
            check(rc, "sbm_match_batch_host_verified");
            for (int f = 0; f < count; ++f) {
                std::vector<VerifiedMatch>& o = out[(size_t)(first + f)];
                for (int32_t i = 0; i < cnt[2 * (size_t)f]; ++i) {
                    const sbm_match_rec& r = recs[(size_t)f * cap + i];
                    o.push_back(VerifiedMatch{Match(r.x, r.y, r.similarity, flat->class_order[(size_t)r.class_idx], r.template_id), scores[(size_t)f * cap + i]});
                }
            }
            break;
        }
    }
    return out;
}

} // namespace line2Dup
