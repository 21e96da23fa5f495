// train_batch_time.cpp — wall time of training 64 templates of 128 x 128 BGR through the facade: a loop of
// Detector::addTemplate, or (without -DLOOP_ONLY, which builds against a tree that has no addTemplates) one
// Detector::addTemplates.  Prints one line per repetition: "<mode> <ms> <templates>".  A run of its own per mode and tree;
// alternate the runs and compare medians (profiles/train_batch.txt).
//   g++ -std=c++14 -O2 [-DLOOP_ONLY] -o train_batch_time tools/train_batch_time.cpp -L shape_based_matching_amd -lsbm_facade -lsbm_hip \
//       -Wl,-rpath,$PWD/shape_based_matching_amd
//   train_batch_time loop|batch <repetitions> [num_features]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/line2Dup.h"

using namespace cv;

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const bool batch = !strcmp(argv[1], "batch");
    const int reps = atoi(argv[2]), nf = argc > 3 ? atoi(argv[3]) : 63;
    std::vector<Mat> sources, masks;
    for (int k = 0; k < 64; ++k) { // a bright rectangle of varying place and size on a dark, slightly textured ground
        Mat img(128, 128, CV_8UC3);
        const int x0 = 16 + k % 8, y0 = 16 + k / 8, w = 64 + (k * 5) % 24, h = 64 + (k * 3) % 24;
        for (int y = 0; y < 128; ++y)
            for (int x = 0; x < 128; ++x) {
                const bool in = x >= x0 && x < x0 + w && y >= y0 && y < y0 + h;
                for (int c = 0; c < 3; ++c) img.ptr(y)[3 * x + c] = (uchar)((in ? 210 : 20) + ((x * 7 + y * 13 + c * 5 + k) % 11));
            }
        sources.push_back(img);
        masks.push_back(Mat());
    }
    for (int r = 0; r < reps + 1; ++r) { // repetition 0 warms the contexts up and is not printed
        line2Dup::Detector detector(nf, {4, 8});
        const auto t0 = std::chrono::steady_clock::now();
        int made = 0;
        if (batch) {
#ifndef LOOP_ONLY
            for (int id : detector.addTemplates(sources, "shapes", masks)) made += id >= 0;
#else
            return 2;
#endif
        } else {
            for (size_t k = 0; k < sources.size(); ++k) made += detector.addTemplate(sources[k], "shapes", masks[k]) >= 0;
        }
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (r) printf("%s %.3f %d\n", batch ? "batch" : "loop", ms, made);
    }
    return 0;
}
