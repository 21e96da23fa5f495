// TEST INFRASTRUCTURE: a driver for line2Dup::verify_patch_of (shape_based_matching_amd/facade/line2Dup_verify_patch.h, the
// body of Detector::verifyPatch), compiled by tests/test_facade_verify_patch.py with facade/cvlite.cpp alone: no engine.
//   driver <rows> <cols> <kind> <sscale> <orientation> <tl_x> <tl_y> <width> <height>
// The fiducial image is made here: kind 0 the ramp 2 * c + r, kind 1 the pattern (r * 37 + c * 101 + (r * c) % 13) & 255.
// Prints "<rows> <cols>" of the patch and its bytes in hex, row by row; "0 0" for an empty patch.
#include <cstdio>
#include <cstdlib>

#include "line2Dup_verify_patch.h"

int main(int argc, char** argv)
{
    if (argc != 10) return 2;
    const int rows = atoi(argv[1]), cols = atoi(argv[2]), kind = atoi(argv[3]);
    cv::Mat img(rows, cols, CV_8UC1);
    for (int r = 0; r < rows; ++r)
        for (int c = 0; c < cols; ++c) img.at<cv::uchar>(r, c) = (cv::uchar)(kind == 0 ? 2 * c + r : (r * 37 + c * 101 + (r * c) % 13) & 255);
    line2Dup::Template t0;
    t0.sscale = (float)atof(argv[4]);
    t0.orientation = (float)atof(argv[5]);
    t0.tl_x = atoi(argv[6]);
    t0.tl_y = atoi(argv[7]);
    t0.width = atoi(argv[8]);
    t0.height = atoi(argv[9]);
    const cv::Mat p = line2Dup::verify_patch_of(t0, img);
    printf("%d %d\n", p.rows, p.cols);
    for (int r = 0; r < p.rows; ++r) {
        for (int c = 0; c < p.cols; ++c) printf("%02x", p.at<cv::uchar>(r, c));
        printf("\n");
    }
    return 0;
}
