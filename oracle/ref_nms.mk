# The reference's own NMS, compiled on stand-in headers: oracle/ref_nms_driver.cpp, which includes the reference's
# nms.hpp from the reference tree (-I), against oracle/ref_cv/ (our own minimal cv::, not the product's include/).
# Output: oracle/_ref/ref_nms, checked by tests/test_reference_nms.py.  Plain -O2 without fast-math and without
# contraction: jaccardDistance__'s mixed int/double arithmetic, the float conversion and the `> 0.5` test on the
# float threshold are the ones written.
# Nothing of the reference is copied: its header is read where it lies.  include/ is not on the path (the product
# has a header of the same name).  What stays unpinned is the stand-in's cv::Rect_ (area(), operator&): our
# restatement of OpenCV's documented behaviour, OpenCV itself not being available.
# The reference tree: SBM_REFERENCE, else the location tools/make_fixtures.py reads too.  Where it is absent nothing is
# done, and a binary built earlier is kept.
CXX           ?= g++
HERE          := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
SBM_REFERENCE ?= /root/reference
OUT           := $(HERE)_ref/ref_nms
DRIVER        := $(HERE)ref_nms_driver.cpp
STANDIN       := $(wildcard $(HERE)ref_cv/*.hpp $(HERE)ref_cv/opencv2/*.hpp $(HERE)ref_cv/opencv2/*/*.hpp)

ifneq ($(wildcard $(SBM_REFERENCE)/nms.hpp),)
all: $(OUT)
$(OUT): $(SBM_REFERENCE)/nms.hpp $(DRIVER) $(STANDIN)
	mkdir -p $(HERE)_ref
	rm -f $@
	$(CXX) -std=c++14 -O2 -fno-fast-math -ffp-contract=off $(DRIVER) \
	    -I $(SBM_REFERENCE) -I $(HERE)ref_cv -o $@ \
	    2> $@.log || { cat $@.log; rm -f $@; exit 1; }
else
all:
	@echo "oracle/ref_nms.mk: no reference tree at $(SBM_REFERENCE): oracle/_ref/ref_nms not (re)built"
endif
.PHONY: all
