# The reference's own match half, compiled on stand-in headers: the reference's line2Dup.cpp with
# oracle/ref_match_driver.cpp appended, against oracle/ref_cv/ (our own minimal cv:: and csv.hpp, not the product's
# include/) and the reference's MIPP.  Output: oracle/_ref/ref_match_{scalar,sse42,avx2}, the three code paths MIPP
# selects on x86 (the AVX2 build is what the reference's -march=native gives on a current host), checked by
# tests/test_reference_match_half.py and, on the GPU, tests/test_gpu_reference_match.py.
# The source is read from the reference tree and piped to the compiler; nothing of it is copied.  -iquote makes the
# reference's own line2Dup.h the one its quoted #include finds; include/ is not on the path (the product header has
# the same name).  No -fopenmp: matchClass's raw list comes out in the serial order.
# The reference tree: SBM_REFERENCE, else the location tools/make_fixtures.py reads too.  Where it is absent nothing is
# done, and binaries built earlier are kept.
CXX           ?= g++
HERE          := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
SBM_REFERENCE ?= /root/reference
OUTDIR        := $(HERE)_ref
DRIVER        := $(HERE)ref_match_driver.cpp
STANDIN       := $(wildcard $(HERE)ref_cv/*.hpp $(HERE)ref_cv/opencv2/*.hpp $(HERE)ref_cv/opencv2/*/*.hpp)
FLAGS_scalar  := -DMIPP_NO_INTRINSICS
FLAGS_sse42   := -msse4.2
FLAGS_avx2    := -mavx2
VARIANTS      := scalar sse42 avx2

ifneq ($(wildcard $(SBM_REFERENCE)/line2Dup.cpp),)
all: $(addprefix $(OUTDIR)/ref_match_,$(VARIANTS))
$(OUTDIR)/ref_match_%: $(SBM_REFERENCE)/line2Dup.cpp $(SBM_REFERENCE)/line2Dup.h $(DRIVER) $(STANDIN)
	mkdir -p $(OUTDIR)
	rm -f $@
	cat $(SBM_REFERENCE)/line2Dup.cpp $(DRIVER) | $(CXX) -std=c++14 -O3 $(FLAGS_$*) -x c++ - \
	    -iquote $(SBM_REFERENCE) -I $(SBM_REFERENCE)/MIPP -I $(HERE)ref_cv -o $@ -lstdc++fs \
	    2> $@.log || { cat $@.log; rm -f $@; exit 1; }
else
all:
	@echo "oracle/ref_match.mk: no reference tree at $(SBM_REFERENCE): oracle/_ref/ref_match_* not (re)built"
endif
.PHONY: all
