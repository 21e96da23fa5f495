# The drop-in check of the facade: the reference's own caller, test.cpp, compiled UNCHANGED against include/line2Dup.h
# and linked against libsbm_facade.so.  Output: oracle/_ref/ref_test_cpp (+ the compiler's messages in
# oracle/_ref/ref_test_cpp.log), checked by tests/test_reference_caller.py.
# The source is read from the reference tree and piped to the compiler (a quoted #include looks in the including file's
# directory first, so compiling it in place would pick the reference's own header); nothing of it is copied.
# The reference tree: SBM_REFERENCE, else the location tools/make_fixtures.py reads too.  Where it is absent nothing is
# done, and a binary built earlier is kept.
CXX           ?= g++
HERE          := $(dir $(abspath $(lastword $(MAKEFILE_LIST))))
PKG           := $(HERE)../shape_based_matching_amd
SBM_REFERENCE ?= /root/reference
OUT           := $(HERE)_ref/ref_test_cpp
HEADERS       := $(wildcard $(HERE)../include/*.h $(HERE)../include/*.hpp)

ifneq ($(wildcard $(SBM_REFERENCE)/test.cpp),)
all: $(OUT)
$(OUT): $(SBM_REFERENCE)/test.cpp $(HEADERS) $(PKG)/libsbm_facade.so $(PKG)/libsbm_hip.so
	mkdir -p $(HERE)_ref
	rm -f $@
	$(CXX) -std=c++14 -x c++ -I $(HERE)../include - -o $@ -L $(PKG) -lsbm_facade -lsbm_hip \
	    -Wl,-rpath,'$$ORIGIN/../../shape_based_matching_amd' -Wl,-rpath-link,$(PKG) -lstdc++fs \
	    < $(SBM_REFERENCE)/test.cpp 2> $@.log || { cat $@.log; rm -f $@; exit 1; }
else
all:
	@echo "oracle/ref_caller.mk: no reference tree at $(SBM_REFERENCE): oracle/_ref/ref_test_cpp not (re)built"
endif
.PHONY: all
