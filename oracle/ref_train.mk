# The reference's own training half, compiled on stand-in headers: the reference's line2Dup.cpp with
# oracle/ref_train_driver.cpp appended, against oracle/ref_cv/ (our own minimal cv:: and csv.hpp, not the product's
# include/) and the reference's MIPP headers, which line2Dup.h includes.  Output: oracle/_ref/ref_train, checked by
# tests/test_reference_train_half.py and, on the GPU, tests/test_gpu_train_batch.py.  One variant: extractTemplate,
# selectScatteredFeatures and cropTemplates use no MIPP (-DMIPP_NO_INTRINSICS keeps the unused match half of the
# translation unit independent of the build host's CPU).  Plain -O2 without fast-math: the float comparisons of the
# scan, the sort and the distance test are the ones written.
# The source is read from the reference tree and piped to the compiler; nothing of it is copied.  -iquote makes the
# reference's own line2Dup.h the one its quoted #include finds; include/ is not on the path.
# The reference tree: SBM_REFERENCE, else the location tools/make_fixtures.py reads too.  Where it is absent nothing is
# done, and a binary built earlier is kept.
CXX           ?= g++
HERE          := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
SBM_REFERENCE ?= /root/reference
OUT           := $(HERE)_ref/ref_train
DRIVER        := $(HERE)ref_train_driver.cpp
STANDIN       := $(wildcard $(HERE)ref_cv/*.hpp $(HERE)ref_cv/opencv2/*.hpp $(HERE)ref_cv/opencv2/*/*.hpp)

ifneq ($(wildcard $(SBM_REFERENCE)/line2Dup.cpp),)
all: $(OUT)
$(OUT): $(SBM_REFERENCE)/line2Dup.cpp $(SBM_REFERENCE)/line2Dup.h $(DRIVER) $(STANDIN)
	mkdir -p $(HERE)_ref
	rm -f $@
	cat $(SBM_REFERENCE)/line2Dup.cpp $(DRIVER) | $(CXX) -std=c++14 -O2 -fno-fast-math -DMIPP_NO_INTRINSICS -x c++ - \
	    -iquote $(SBM_REFERENCE) -I $(SBM_REFERENCE)/MIPP -I $(HERE)ref_cv -o $@ -lstdc++fs \
	    2> $@.log || { cat $@.log; rm -f $@; exit 1; }
else
all:
	@echo "oracle/ref_train.mk: no reference tree at $(SBM_REFERENCE): oracle/_ref/ref_train not (re)built"
endif
.PHONY: all
