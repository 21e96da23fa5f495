// Stand-in for OpenCV 4's imgproc header (test infrastructure; see opencv2/core/core.hpp).  The filters and transforms
// line2Dup.cpp names are declared there; the gradient half's throw when called on an image, erode has the one form
// extractTemplate uses.
#ifndef SBM_REF_CV_IMGPROC_HPP
#define SBM_REF_CV_IMGPROC_HPP
#include "core/core.hpp"
#endif
