// train_ragged_time.cpp — wall time of the training scale sweep of test.cpp:scale_test("train") through the facade: the loop
// of Detector::addTemplate(shapes.src_of(info), class_id, shapes.mask_of(info), ...) against one
// shapeInfo_producer::addTemplates (device resize + ragged batched training), alternating in one process after a warm-up
// of each.  Prints one line per repetition, "<mode> <ms> <templates>", then the medians and the spreads
// (profiles/train_ragged.txt).
//   g++ -std=c++14 -O2 -o train_ragged_time tools/train_ragged_time.cpp -L shape_based_matching_amd -lsbm_facade -lsbm_hip
//       -Wl,-rpath,$PWD/shape_based_matching_amd          (one command line)
//   train_ragged_time <image.ppm> <num_features> <scale_lo> <scale_hi> <scale_step> <repetitions>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/line2Dup.h"

using namespace cv;

int main(int argc, char** argv)
{
    if (argc < 7) return 2;
    Mat img = imread(argv[1], IMREAD_UNCHANGED);
    if (img.empty()) return 1;
    const int nf = atoi(argv[2]), reps = atoi(argv[6]);
    shape_based_matching::shapeInfo_producer shapes(img);
    shapes.scale_range = {(float)atof(argv[3]), (float)atof(argv[4])};
    shapes.scale_step = (float)atof(argv[5]);
    shapes.produce_infos();
    std::vector<float> sscales;
    for (auto& info : shapes.infos) sscales.push_back((float)int(nf * info.scale));
    std::vector<double> ms[2];
    for (int r = 0; r < 2 * (reps + 1); ++r) { // the first of each mode warms up and is not counted
        const int batch = r & 1;
        line2Dup::Detector detector(nf, {4, 8});
        const auto t0 = std::chrono::steady_clock::now();
        int made = 0;
        if (batch) {
            for (int id : shapes.addTemplates(detector, "circle", shapes.infos, sscales)) made += id >= 0;
        } else {
            for (auto& info : shapes.infos) made += detector.addTemplate(shapes.src_of(info), "circle", shapes.mask_of(info), int(nf * info.scale)) >= 0;
        }
        const double t = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (r < 2) continue;
        printf("%s %.3f %d\n", batch ? "batch" : "loop", t, made);
        ms[batch].push_back(t);
    }
    for (int b = 0; b < 2; ++b) {
        std::sort(ms[b].begin(), ms[b].end());
        if (ms[b].empty()) continue;
        printf("%s infos %zu median %.3f min %.3f max %.3f\n", b ? "batch" : "loop", shapes.infos.size(), ms[b][ms[b].size() / 2], ms[b].front(), ms[b].back());
    }
    return 0;
}
