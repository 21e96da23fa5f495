// line2Dup_verify_patch.h — the fiducial patch of a template, header-only so that it builds without the engine
// (tests/test_facade_verify_patch.py compiles it with cvlite.cpp alone); Detector::verifyPatch (line2Dup_verify.cpp) is
// this function.
//
// Reference: test_jabil.cpp:187-191 -- the fiducial image through rotateScaleImage(img, sscale, orientation)
// (utils.cpp:157-187: cv::resize by the scale when |scale - 1| > FLT_EPSILON, then cv::rotate by the flag of the integer
// angle: 90 / -270 clockwise, 270 / -90 counter-clockwise, 180 / -180 half a turn, anything else none), then the crop
// Rect(tl_x, tl_y, width, height).  Where that crop leaves the image the reference throws; here the patch is empty.
#pragma once
#include "../../include/line2Dup.h"

#include <cfloat>
#include <cmath>

namespace line2Dup {

inline cv::Mat verify_patch_of(const Template& t0, const cv::Mat& fiducial_gray)
{
    if (fiducial_gray.empty() || fiducial_gray.type() != CV_8UC1) return cv::Mat();
    cv::Mat img = fiducial_gray;
    if (std::abs(t0.sscale - 1.0) > FLT_EPSILON) {
        cv::Mat scaled;
        cv::resize(img, scaled, cv::Size(), t0.sscale, t0.sscale);
        img = scaled;
    }
    const int angle = static_cast<int>(t0.orientation);
    int flag = -1;
    if (angle == 90 || angle == -270) flag = cv::ROTATE_90_CLOCKWISE;
    else if (angle == 270 || angle == -90) flag = cv::ROTATE_90_COUNTERCLOCKWISE;
    else if (angle == 180 || angle == -180) flag = cv::ROTATE_180;
    if (flag >= 0) {
        cv::Mat turned;
        cv::rotate(img, turned, flag);
        img = turned;
    }
    if (t0.width <= 0 || t0.height <= 0 || t0.tl_x < 0 || t0.tl_y < 0 || t0.tl_x + t0.width > img.cols || t0.tl_y + t0.height > img.rows)
        return cv::Mat();
    return img(cv::Rect(t0.tl_x, t0.tl_y, t0.width, t0.height)).clone();
}

} // namespace line2Dup
