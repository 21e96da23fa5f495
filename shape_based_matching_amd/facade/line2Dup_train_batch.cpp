// line2Dup_train_batch.cpp — Detector::addTemplates: addTemplate for a list of sources over the engine's batched training
// entry point (sbm_train_batch).  A translation unit of its own: it is the only part of the facade that needs that entry point.
#include "../../include/line2Dup.h"
#include "../../include/sbm.h"

#include <algorithm>
#include <cstring>
#include <iostream>
#include <map>
#include <mutex>
#include <tuple>

using namespace cv;

namespace {

void check(int rc, const char* what)
{
    if (rc != 0) CV_Error(rc == SBM_ERR_INVALID ? Error::StsBadArg : Error::StsError, std::string(what) + ": " + sbm_last_error());
}

// The context of the batched training path (Detector::addTemplates): sbm_train_batch takes the pyramid's depth and the
// weak threshold from its context, so this one is made for the detector's and kept until a detector with other values asks.
// Device 0, as the context of addTemplate's stage calls.  Training mutates the detector and is not concurrent with anything else on it; the mutex
// guards the contexts of different detectors against each other.
std::mutex g_train_mu;
sbm_ctx* train_ctx(const std::vector<int>& T, int levels, float weak_threshold)
{
    static sbm_ctx* ctx = nullptr;
    static sbm_config have;
    sbm_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.n_levels = levels;
    for (int l = 0; l < levels; ++l) cfg.T[l] = T[(size_t)l];
    cfg.weak_threshold = weak_threshold;
    cfg.device_id = 0;
    cfg.max_candidates = 1024;
    if (ctx && memcmp(&cfg, &have, sizeof cfg) != 0) {
        sbm_destroy(ctx);
        ctx = nullptr;
    }
    if (!ctx) {
        check(sbm_create(&cfg, &ctx), "sbm_create");
        have = cfg;
    }
    return ctx;
}

} // namespace

namespace line2Dup {

// addTemplate for a list of sources (an extension: the reference's callers train in bulk, test_jabil.cpp:46-118).  The
// sources are grouped by geometry and every group goes through sbm_train_batch -- gradients, maxima, tie resolution,
// selection and cropTemplates on the device, no round trip per template -- in sub-batches bounded by a scratch budget.
// Element k is what the k-th call of a loop of addTemplate returns, and the detector afterwards is the loop's.
std::vector<int> Detector::addTemplates(const std::vector<Mat>& sources, const std::string& class_id, const std::vector<Mat>& object_masks,
                                        const std::vector<float>& sscales, const std::vector<float>& orientations, int tagFieldID,
                                        std::string fiducial_src, int num_features)
{
    const size_t n = sources.size();
    CV_Assert(object_masks.empty() || object_masks.size() == n);
    CV_Assert(sscales.empty() || sscales.size() == n);
    CV_Assert(orientations.empty() || orientations.size() == n);
    CV_Assert(pyramid_levels >= 1 && pyramid_levels <= SBM_MAX_LEVELS && (int)T_at_level.size() >= pyramid_levels);
    std::vector<TemplatePyramid>& template_pyramids = class_templates[class_id];
    std::vector<int> ids(n, -1);
    if (n == 0) return ids;
    const int nf = num_features > 0 ? num_features : (int)modality->num_features;
    std::map<std::tuple<int, int, int>, std::vector<size_t>> groups; // (rows, cols, type) -> sources, in input order
    for (size_t k = 0; k < n; ++k) {
        const Mat& src = sources[k];
        CV_Assert(!src.empty() && src.depth() == CV_8U && (src.channels() == 1 || src.channels() == 3));
        if (!object_masks.empty() && !object_masks[k].empty())
            CV_Assert(object_masks[k].type() == CV_8UC1 && object_masks[k].size() == src.size());
        groups[std::make_tuple(src.rows, src.cols, src.type())].push_back(k);
    }
    std::vector<TemplatePyramid> made(n);
    std::vector<char> ok(n, 0);
    std::lock_guard<std::mutex> lock(g_train_mu);
    sbm_ctx* ctx = train_ctx(T_at_level, pyramid_levels, modality->weak_threshold);
    for (const auto& g : groups) {
        const int rows = std::get<0>(g.first), cols = std::get<1>(g.first), ch = CV_MAT_CN(std::get<2>(g.first));
        // no two accepted maxima within a 3 x 3 cell: the most features an image can have, level by level
        int64_t feat_cap = 0, pixels = 0;
        for (int l = 0; l < pyramid_levels; ++l) {
            feat_cap += (int64_t)(((rows >> l) + 2) / 3) * (((cols >> l) + 2) / 3);
            pixels += (int64_t)(rows >> l) * (cols >> l);
        }
        // the engine's scratch per image: the image and its float / byte planes per pixel, the lists per candidate
        const int64_t per_image = pixels * (ch + 11) + feat_cap * 64 + 4096, budget = (int64_t)256 << 20;
        const size_t sub = (size_t)std::max<int64_t>(1, std::min<int64_t>(budget / per_image, 4096));
        for (size_t first = 0; first < g.second.size(); first += sub) {
            const size_t m = std::min(sub, g.second.size() - first);
            std::vector<Mat> keep; // continuous copies of views
            std::vector<const uint8_t*> imgs(m), masks(m, nullptr);
            bool any_mask = false;
            for (size_t i = 0; i < m; ++i) {
                const size_t k = g.second[first + i];
                Mat src = sources[k];
                if (!src.isContinuous()) keep.push_back(src = src.clone());
                imgs[i] = src.data;
                if (!object_masks.empty() && !object_masks[k].empty()) {
                    Mat mk = object_masks[k];
                    if (!mk.isContinuous()) keep.push_back(mk = mk.clone());
                    masks[i] = mk.data;
                    any_mask = true;
                }
            }
            std::vector<sbm_template_level> levels(m * (size_t)pyramid_levels);
            std::vector<sbm_train_feature> feats(m * (size_t)feat_cap);
            std::vector<int32_t> status(m * 2);
            check(sbm_train_batch(ctx, imgs.data(), (int)m, rows, cols, cols * ch, ch, any_mask ? masks.data() : nullptr, modality->strong_threshold, nf,
                                  levels.data(), feats.data(), feat_cap, status.data()),
                  "sbm_train_batch");
            for (size_t i = 0; i < m; ++i) {
                const size_t k = g.second[first + i];
                if (status[2 * i] == 1) {
                    std::cout << "extractTemplate: too few candidate features at pyramid level " << status[2 * i + 1] << ", giving up on this template"
                              << std::endl;
                    continue;
                }
                CV_Assert(status[2 * i] == 0);
                TemplatePyramid tp((size_t)pyramid_levels);
                for (int l = 0; l < pyramid_levels; ++l) {
                    const sbm_template_level& lv = levels[i * (size_t)pyramid_levels + (size_t)l];
                    Template& t = tp[(size_t)l];
                    t.width = lv.width;
                    t.height = lv.height;
                    t.tl_x = lv.tl_x;
                    t.tl_y = lv.tl_y;
                    t.pyramid_level = lv.pyramid_level;
                    t.sscale = sscales.empty() ? -1.0f : sscales[k];
                    t.orientation = orientations.empty() ? -1.0f : orientations[k];
                    t.tagFieldID = tagFieldID;
                    t.fiducial_src = fiducial_src;
                    t.features.resize((size_t)lv.n_features);
                    const sbm_train_feature* f = feats.data() + i * (size_t)feat_cap + (size_t)lv.feature_offset;
                    for (int j = 0; j < lv.n_features; ++j) {
                        Feature& o = t.features[(size_t)j];
                        o.x = f[j].x;
                        o.y = f[j].y;
                        o.label = f[j].label;
                        o.theta = f[j].theta;
                    }
                }
                made[k] = tp;
                ok[k] = 1;
            }
        }
    }
    bool any = false;
    for (size_t k = 0; k < n; ++k) { // ids in input order, whatever the grouping; a failed template takes none
        if (!ok[k]) continue;
        ids[k] = static_cast<int>(template_pyramids.size());
        template_pyramids.push_back(made[k]);
        any = true;
    }
    if (any) templatesChanged();
    return ids;
}

} // namespace line2Dup
