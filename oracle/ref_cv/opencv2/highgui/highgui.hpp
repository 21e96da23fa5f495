// Stand-in for OpenCV 4's highgui header (test infrastructure; see opencv2/core/core.hpp).  line2Dup.cpp uses nothing
// from it.
#ifndef SBM_REF_CV_HIGHGUI_HPP
#define SBM_REF_CV_HIGHGUI_HPP
#include "../core/core.hpp"
#endif
