# Builds the C++ tests of the robust absolute pose (host compiler only):
#   absolute_pose_block_test      csrc/absolute_pose_block.h compiled for the host
#   absolute_pose_block_test_san  the same under AddressSanitizer + UBSan (a
#                                 stand-alone program; never loaded into Python)
#   absolute_pose_test            the facade (include/colmap_amd/pose.h) against libmi_ba.so
# Used as `make -f absolute_pose.mk TARGET` from this directory.
# -ffp-contract=off: the block header recomputes residuals and relies on their
# bits being the same wherever they are inlined, on any host architecture.
ROOT := $(abspath ../..)
LIBDIR := $(ROOT)/semantic-bundle-adjustment-colmap_amd
INC := $(ROOT)/include/colmap_amd
CXX ?= g++
BLOCK_DEPS := absolute_pose_block_test.cc $(LIBDIR)/csrc/absolute_pose_block.h $(LIBDIR)/csrc/ba_math.h

all: absolute_pose_block_test absolute_pose_block_test_san absolute_pose_test

absolute_pose_block_test: $(BLOCK_DEPS)
	$(CXX) -O2 -std=c++17 -Wall -ffp-contract=off -fopenmp -o $@ $<

absolute_pose_block_test_san: $(BLOCK_DEPS)
	$(CXX) -O1 -g -std=c++17 -Wall -Wno-unknown-pragmas -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -o $@ $<

absolute_pose_test: absolute_pose_test.cc $(INC)/pose.h $(INC)/bundle_adjustment.h $(ROOT)/include/mi_ba.h \
	$(LIBDIR)/csrc/absolute_pose_block.h $(LIBDIR)/csrc/ba_math.h $(LIBDIR)/libmi_ba.so
	$(CXX) -O2 -std=c++17 -Wall -ffp-contract=off -I$(ROOT)/include -o $@ $< -L$(LIBDIR) -lmi_ba -Wl,-rpath,$(LIBDIR)

clean:
	rm -f absolute_pose_block_test absolute_pose_block_test_san absolute_pose_test
.PHONY: all clean
