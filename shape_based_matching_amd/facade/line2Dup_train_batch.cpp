// line2Dup_train_batch.cpp — Detector::addTemplates: addTemplate for a list of sources over the engine's batched training
// entry points (sbm_train_batch for one geometry, sbm_train_ragged for any list), Detector::addTemplatesScaled and
// shapeInfo_producer::addTemplates over the device scale sweep (sbm_train_sweep).  A translation unit of its own: it is the
// only part of the facade that needs those entry points.
#include "../../include/line2Dup.h"
#include "../../include/sbm.h"

#include <algorithm>
#include <cmath>
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

// no two accepted maxima within a 3 x 3 cell: the most features an image can have, level by level; and the engine's
// scratch for it: the image and its float / byte planes per pixel, the lists per candidate
void train_bounds(int rows, int cols, int ch, int levels, int64_t* feat_cap, int64_t* scratch)
{
    int64_t cap = 0, pixels = 0;
    for (int l = 0; l < levels; ++l) {
        cap += (int64_t)(((rows >> l) + 2) / 3) * (((cols >> l) + 2) / 3);
        pixels += (int64_t)(rows >> l) * (cols >> l);
    }
    *feat_cap = cap;
    *scratch = pixels * (ch + 11) + cap * 64 + 4096;
}

const int64_t kTrainBudget = (int64_t)256 << 20;

} // namespace

namespace line2Dup {

// One trained image as a TemplatePyramid; false (and addTemplate's message) where the engine reports too few candidates.
static bool train_result(int pyramid_levels, const sbm_template_level* levels, const sbm_train_feature* block, const int32_t* status, float sscale,
                         float orientation, int tagFieldID, const std::string& fiducial_src, std::vector<Template>& tp)
{
    if (status[0] == 1) {
        std::cout << "extractTemplate: too few candidate features at pyramid level " << status[1] << ", giving up on this template" << std::endl;
        return false;
    }
    CV_Assert(status[0] == 0);
    tp.assign((size_t)pyramid_levels, Template());
    for (int l = 0; l < pyramid_levels; ++l) {
        const sbm_template_level& lv = levels[l];
        Template& t = tp[(size_t)l];
        t.width = lv.width;
        t.height = lv.height;
        t.tl_x = lv.tl_x;
        t.tl_y = lv.tl_y;
        t.pyramid_level = lv.pyramid_level;
        t.sscale = sscale;
        t.orientation = orientation;
        t.tagFieldID = tagFieldID;
        t.fiducial_src = fiducial_src;
        t.features.resize((size_t)lv.n_features);
        const sbm_train_feature* f = block + (size_t)lv.feature_offset;
        for (int j = 0; j < lv.n_features; ++j) {
            Feature& o = t.features[(size_t)j];
            o.x = f[j].x;
            o.y = f[j].y;
            o.label = f[j].label;
            o.theta = f[j].theta;
        }
    }
    return true;
}

// addTemplate for a list of sources (an extension: the reference's callers train in bulk, test_jabil.cpp:46-118).  The
// sources are grouped by geometry and every group goes through sbm_train_batch -- gradients, maxima, tie resolution,
// selection and cropTemplates on the device, no round trip per template -- in sub-batches bounded by a scratch budget.
// Element k is what the k-th call of a loop of addTemplate returns, and the detector afterwards is the loop's.
std::vector<int> Detector::addTemplates(const std::vector<Mat>& sources, const std::string& class_id, const std::vector<Mat>& object_masks,
                                        const std::vector<float>& sscales, const std::vector<float>& orientations, int tagFieldID,
                                        std::string fiducial_src, int num_features, const std::vector<int>& num_features_each)
{
    const size_t n = sources.size();
    CV_Assert(num_features_each.empty() || num_features_each.size() == n);
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
    const bool ragged = groups.size() > 1 || !num_features_each.empty();
    // Any list: every source with its own size and count through sbm_train_ragged, in input order, in sub-batches whose
    // scratch, summed per image, stays under the budget.
    for (size_t first = 0; ragged && first < n;) {
        std::vector<Mat> keep; // continuous copies of views
        std::vector<sbm_train_image> imgs;
        int64_t feats_total = 0, scratch_total = 0;
        const int ch = sources[first].channels();
        size_t m = 0;
        for (; first + m < n && m < 4096; ++m) {
            const size_t k = first + m;
            Mat src = sources[k];
            if (src.channels() != ch) break; // a call's images share the number of channels
            int64_t cap, scratch;
            train_bounds(src.rows, src.cols, ch, pyramid_levels, &cap, &scratch);
            if (m > 0 && scratch_total + scratch > kTrainBudget) break;
            if (!src.isContinuous()) keep.push_back(src = src.clone());
            sbm_train_image im;
            memset(&im, 0, sizeof im);
            im.img = src.data;
            if (!object_masks.empty() && !object_masks[k].empty()) {
                Mat mk = object_masks[k];
                if (!mk.isContinuous()) keep.push_back(mk = mk.clone());
                im.mask = mk.data;
            }
            im.rows = src.rows, im.cols = src.cols, im.stride = src.cols * ch;
            const int each = num_features_each.empty() ? 0 : num_features_each[k];
            im.num_features = each > 0 ? each : nf; // addTemplate: a count <= 0 means the detector's
            im.feat_first = feats_total, im.feat_cap = cap;
            imgs.push_back(im);
            feats_total += cap;
            scratch_total += scratch;
        }
        std::vector<sbm_template_level> levels(m * (size_t)pyramid_levels);
        std::vector<sbm_train_feature> feats((size_t)std::max<int64_t>(feats_total, 1));
        std::vector<int32_t> status(m * 2);
        check(sbm_train_ragged(ctx, imgs.data(), (int)m, ch, modality->strong_threshold, levels.data(), feats.data(), status.data()), "sbm_train_ragged");
        for (size_t i = 0; i < m; ++i) {
            const size_t k = first + i;
            ok[k] = train_result(pyramid_levels, levels.data() + i * (size_t)pyramid_levels, feats.data() + imgs[i].feat_first, status.data() + 2 * i,
                                 sscales.empty() ? -1.0f : sscales[k], orientations.empty() ? -1.0f : orientations[k], tagFieldID, fiducial_src, made[k]);
        }
        first += m;
    }
    for (const auto& g : groups) {
        if (ragged) break;
        const int rows = std::get<0>(g.first), cols = std::get<1>(g.first), ch = CV_MAT_CN(std::get<2>(g.first));
        int64_t feat_cap, per_image;
        train_bounds(rows, cols, ch, pyramid_levels, &feat_cap, &per_image);
        const int64_t budget = kTrainBudget;
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
                ok[k] = train_result(pyramid_levels, levels.data() + i * (size_t)pyramid_levels, feats.data() + i * (size_t)feat_cap, status.data() + 2 * i,
                                     sscales.empty() ? -1.0f : sscales[k], orientations.empty() ? -1.0f : orientations[k], tagFieldID, fiducial_src, made[k]);
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

// The scale sweep of one source over sbm_train_sweep: uploaded once, resized on the device, trained as one ragged batch
// (in sub-batches under the scratch budget).  The loop of addTemplate(resize(source, s), class_id, resize(mask, s) > 0, ...).
std::vector<int> Detector::addTemplatesScaled(const Mat& source, const std::string& class_id, const Mat& object_mask, const std::vector<float>& scales,
                                              const std::vector<float>& sscales, const std::vector<float>& orientations, int tagFieldID,
                                              std::string fiducial_src, const std::vector<int>& num_features_each)
{
    const size_t n = scales.size();
    CV_Assert(sscales.empty() || sscales.size() == n);
    CV_Assert(orientations.empty() || orientations.size() == n);
    CV_Assert(num_features_each.empty() || num_features_each.size() == n);
    CV_Assert(pyramid_levels >= 1 && pyramid_levels <= SBM_MAX_LEVELS && (int)T_at_level.size() >= pyramid_levels);
    CV_Assert(!source.empty() && source.depth() == CV_8U && (source.channels() == 1 || source.channels() == 3));
    CV_Assert(object_mask.empty() || (object_mask.type() == CV_8UC1 && object_mask.size() == source.size()));
    std::vector<TemplatePyramid>& template_pyramids = class_templates[class_id];
    std::vector<int> ids(n, -1);
    if (n == 0) return ids;
    const Mat src = source.isContinuous() ? source : source.clone();
    const Mat mask = object_mask.empty() || object_mask.isContinuous() ? object_mask : object_mask.clone();
    const int ch = src.channels();
    std::lock_guard<std::mutex> lock(g_train_mu);
    sbm_ctx* ctx = train_ctx(T_at_level, pyramid_levels, modality->weak_threshold);
    bool any = false;
    for (size_t first = 0; first < n;) {
        std::vector<sbm_train_scale> sc;
        int64_t feats_total = 0, scratch_total = 0;
        size_t m = 0;
        for (; first + m < n && m < 4096; ++m) {
            const size_t k = first + m;
            int32_t dr = 0, dc = 0;
            check(sbm_resize_linear(ctx, src.data, src.rows, src.cols, src.cols * ch, ch, scales[k], scales[k], nullptr, 0, &dr, &dc), "sbm_resize_linear");
            int64_t cap, scratch;
            train_bounds(std::max(dr, 0), std::max(dc, 0), ch, pyramid_levels, &cap, &scratch);
            scratch += (int64_t)std::max(dr, 0) * std::max(dc, 0) * (ch + 1); // the scaled image and mask
            if (m > 0 && scratch_total + scratch > kTrainBudget) break;
            sbm_train_scale s;
            memset(&s, 0, sizeof s);
            s.fx = s.fy = scales[k];
            const int each = num_features_each.empty() ? 0 : num_features_each[k];
            s.num_features = each > 0 ? each : (int)modality->num_features;
            s.feat_first = feats_total, s.feat_cap = cap;
            sc.push_back(s);
            feats_total += cap;
            scratch_total += scratch;
        }
        std::vector<sbm_template_level> levels(m * (size_t)pyramid_levels);
        std::vector<sbm_train_feature> feats((size_t)std::max<int64_t>(feats_total, 1));
        std::vector<int32_t> status(m * 2);
        check(sbm_train_sweep(ctx, src.data, src.rows, src.cols, src.cols * ch, ch, mask.empty() ? nullptr : mask.data, sc.data(), (int)m,
                              modality->strong_threshold, levels.data(), feats.data(), status.data()),
              "sbm_train_sweep");
        for (size_t i = 0; i < m; ++i) {
            const size_t k = first + i;
            TemplatePyramid tp;
            if (!train_result(pyramid_levels, levels.data() + i * (size_t)pyramid_levels, feats.data() + sc[i].feat_first, status.data() + 2 * i,
                              sscales.empty() ? -1.0f : sscales[k], orientations.empty() ? -1.0f : orientations[k], tagFieldID, fiducial_src, tp))
                continue;
            ids[k] = static_cast<int>(template_pyramids.size());
            template_pyramids.push_back(tp);
            any = true;
        }
        first += m;
    }
    if (any) templatesChanged();
    return ids;
}

// The loop of addTemplate_rotate over bases and angles as sbm_train_rotate calls: every base flattened once (its level
// records with packed feature offsets, its features), rotation k of base b in a block of the base's feature count.  One
// call where the whole family's features stay under the budget; otherwise base by base, the angles in runs that do.
std::vector<int> Detector::addTemplates_rotate(const std::string& class_id, const std::vector<int>& zero_ids, const std::vector<float>& thetas,
                                               const std::vector<Point2f>& centers)
{
    const size_t nb = zero_ids.size(), nt = thetas.size();
    CV_Assert(centers.size() == nb);
    CV_Assert(pyramid_levels >= 1 && pyramid_levels <= SBM_MAX_LEVELS && (int)T_at_level.size() >= pyramid_levels);
    std::vector<TemplatePyramid>& template_pyramids = class_templates[class_id];
    const int have = static_cast<int>(template_pyramids.size());
    for (int id : zero_ids) CV_Assert(id >= 0 && id < have);
    std::vector<int> ids;
    if (nb == 0 || nt == 0) return ids;
    const size_t L = (size_t)pyramid_levels;
    std::vector<sbm_template_level> base_levels(nb * L);
    std::vector<std::vector<sbm_train_feature>> base_feats(nb);
    std::vector<int64_t> count(nb, 0);
    int64_t family = 0; // features of all rotations
    for (size_t b = 0; b < nb; ++b) {
        const TemplatePyramid& tp = template_pyramids[(size_t)zero_ids[b]];
        CV_Assert(tp.size() == L);
        for (size_t l = 0; l < L; ++l) {
            sbm_template_level& lv = base_levels[b * L + l];
            lv.width = tp[l].width, lv.height = tp[l].height, lv.tl_x = tp[l].tl_x, lv.tl_y = tp[l].tl_y;
            lv.pyramid_level = (int)l;
            lv.n_features = (int)tp[l].features.size();
            lv.feature_offset = count[b];
            for (const Feature& f : tp[l].features) {
                sbm_train_feature g;
                g.x = f.x, g.y = f.y, g.label = f.label, g.theta = f.theta;
                base_feats[b].push_back(g);
            }
            count[b] += lv.n_features;
        }
        if (base_feats[b].empty()) base_feats[b].resize(1);
        family += count[b] * (int64_t)nt;
    }
    const int64_t budget = kTrainBudget / (int64_t)sizeof(sbm_train_feature);
    std::vector<TemplatePyramid> made(nb * nt);
    std::lock_guard<std::mutex> lock(g_train_mu);
    sbm_ctx* ctx = train_ctx(T_at_level, pyramid_levels, modality->weak_threshold);
    // bases [b0, b1) at the angles [k0, k1): one engine call
    auto run = [&](size_t b0, size_t b1, size_t k0, size_t k1) {
        const size_t m = k1 - k0;
        std::vector<sbm_rotate_base> recs(b1 - b0);
        int64_t first = 0;
        for (size_t b = b0; b < b1; ++b) {
            sbm_rotate_base& r = recs[b - b0];
            memset(&r, 0, sizeof r);
            r.levels = base_levels.data() + b * L;
            r.feats = base_feats[b].data();
            r.center_x = centers[b].x, r.center_y = centers[b].y;
            r.out_first = first, r.out_cap = count[b];
            first += count[b] * (int64_t)m;
        }
        std::vector<sbm_template_level> levels(recs.size() * m * L);
        std::vector<sbm_train_feature> feats((size_t)std::max<int64_t>(first, 1));
        std::vector<int32_t> status(recs.size() * m * 2);
        check(sbm_train_rotate(ctx, recs.data(), (int)recs.size(), thetas.data() + k0, (int)m, levels.data(), feats.data(), status.data()), "sbm_train_rotate");
        for (size_t b = b0; b < b1; ++b)
            for (size_t k = 0; k < m; ++k) {
                const size_t p = (b - b0) * m + k;
                if (status[2 * p] != 0)
                    CV_Error(Error::StsBadArg, cv::format("addTemplates_rotate: template %d at angle %zu is outside the engine's domain (status %d, %d)",
                                                          zero_ids[b], k0 + k, status[2 * p], status[2 * p + 1]));
                TemplatePyramid& tp = made[b * nt + k0 + k];
                tp.assign(L, Template());
                const sbm_train_feature* block = feats.data() + recs[b - b0].out_first + (int64_t)k * recs[b - b0].out_cap;
                for (size_t l = 0; l < L; ++l) {
                    const sbm_template_level& lv = levels[p * L + l];
                    Template& t = tp[l];
                    t.width = lv.width, t.height = lv.height, t.tl_x = lv.tl_x, t.tl_y = lv.tl_y;
                    t.pyramid_level = lv.pyramid_level;
                    t.features.resize((size_t)lv.n_features);
                    const sbm_train_feature* f = block + lv.feature_offset;
                    for (int j = 0; j < lv.n_features; ++j) {
                        Feature& o = t.features[(size_t)j];
                        o.x = f[j].x, o.y = f[j].y, o.label = f[j].label, o.theta = f[j].theta;
                    }
                }
            }
    };
    if (family <= budget) {
        run(0, nb, 0, nt);
    } else {
        for (size_t b = 0; b < nb; ++b) {
            const size_t step = (size_t)std::max<int64_t>(1, std::min<int64_t>((int64_t)nt, budget / std::max<int64_t>(count[b], 1)));
            for (size_t k0 = 0; k0 < nt; k0 += step) run(b, b + 1, k0, std::min(nt, k0 + step));
        }
    }
    for (size_t p = 0; p < made.size(); ++p) { // the loop's order: base by base, angle by angle
        ids.push_back(static_cast<int>(template_pyramids.size()));
        template_pyramids.push_back(std::move(made[p]));
    }
    templatesChanged();
    return ids;
}

} // namespace line2Dup

namespace shape_based_matching {

// 0: no rotation (transform only resizes), 1: 90, 2: 180, 3: 270 -- the branches of transform (line2Dup.h:379-405)
static int rotation_class(float angle)
{
    if (std::abs(angle - 90.0) < ANGLE_TOLERANCE) return 1;
    if (std::abs(angle - 180.0) < ANGLE_TOLERANCE) return 2;
    if (std::abs(angle - 270.0) < ANGLE_TOLERANCE) return 3;
    return 0;
}

static Mat rotated(const Mat& m, int rc)
{
    if (rc == 0 || m.empty()) return m;
    Mat dst;
    cv::rotate(m, dst, rc == 1 ? cv::ROTATE_90_CLOCKWISE : rc == 2 ? cv::ROTATE_180 : cv::ROTATE_90_COUNTERCLOCKWISE);
    return dst;
}

std::vector<int> shapeInfo_producer::addTemplates(line2Dup::Detector& detector, const std::string& class_id, const std::vector<Info>& infos_,
                                                  const std::vector<float>& sscales, const std::vector<float>& orientations, int tagFieldID,
                                                  std::string fiducial_src, const std::vector<int>& num_features_each)
{
    const size_t n = infos_.size();
    CV_Assert(sscales.empty() || sscales.size() == n);
    CV_Assert(orientations.empty() || orientations.size() == n);
    CV_Assert(num_features_each.empty() || num_features_each.size() == n);
    std::vector<int> ids;
    for (size_t first = 0; first < n;) {
        const int rc = rotation_class(infos_[first].angle);
        size_t m = 1;
        while (first + m < n && rotation_class(infos_[first + m].angle) == rc) ++m;
        std::vector<float> scales(m);
        for (size_t i = 0; i < m; ++i) scales[i] = infos_[first + i].scale;
        auto part = [&](const std::vector<float>& v) { return v.empty() ? v : std::vector<float>(v.begin() + (long)first, v.begin() + (long)(first + m)); };
        const std::vector<int> each = num_features_each.empty()
                                          ? num_features_each
                                          : std::vector<int>(num_features_each.begin() + (long)first, num_features_each.begin() + (long)(first + m));
        const std::vector<int> got = detector.addTemplatesScaled(rotated(src, rc), class_id, rotated(mask, rc), scales, part(sscales), part(orientations),
                                                                 tagFieldID, fiducial_src, each);
        ids.insert(ids.end(), got.begin(), got.end());
        first += m;
    }
    return ids;
}

} // namespace shape_based_matching
