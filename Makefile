# Builds the C-ABI HIP library for gfx950 (cross-compiles without a GPU).
#   make            -> scene-net_amd/lib/libscenenet_hip.so
#   make asm        -> build/*.s + resource usage (VGPR/LDS/occupancy) for inspection
HIPCC    ?= /opt/rocm/bin/hipcc
ARCH     ?= gfx950
PKG      := scene-net_amd
SRC      := $(PKG)/csrc
OUT      := $(PKG)/lib
OBJDIR   := build/obj
# EXTRA: e.g. `make -B EXTRA=-DSN_CONV_TIMING` builds the per-workgroup phase clocks tools/conv_timing.py reads
CXXFLAGS := -O3 -std=c++17 -fPIC --offload-arch=$(ARCH) -Iinclude -I$(SRC) -Wall -Wno-unused-function $(EXTRA)
# voxel.hip reproduces numpy's fp64 rounding sequence: never contract a*b+c
FLAGS_voxel := -ffp-contract=off
# metrics.hip: the fp64 value arithmetic is metrics.py's binary_metric_values operation for operation
FLAGS_metrics := -ffp-contract=off
# towers.hip: the stencil's fp64 inclusion test is evaluated in exactly the documented form
FLAGS_towers := -ffp-contract=off
# crops.hip: the disc test's fp64 products and sum are rounded once each, as numpy rounds them
FLAGS_crops := -ffp-contract=off
# dbscan.hip: the neighbour test's fp64 products and sums are rounded once each, in the documented order
FLAGS_dbscan := -ffp-contract=off
# tower_score.hip: centroids, means and distances are fp64 operations rounded once each, in numpy's order
FLAGS_tower_score := -ffp-contract=off
# las.hip: a coordinate is (double)X * scale + offset with the product and the sum rounded once each, as numpy rounds them
FLAGS_las := -ffp-contract=off
# las_write.hip: an integer coordinate is rint((x - offset) / scale) with the difference and the quotient rounded once each, as numpy rounds them
FLAGS_las_write := -ffp-contract=off
# voxel_cloud.hip: a colour is (1 + c) * 255.0 with the sum and the product rounded once each, as numpy rounds them
FLAGS_voxel_cloud := -ffp-contract=off
# thin.hip: bins with K1's fp64 rounding sequence (binning.h) and forms its uniform without a contracted multiply-add
FLAGS_thin := -ffp-contract=off
# voxel_classes.hip: bins with K1's fp64 rounding sequence (binning.h) and forms 255 * c for the rgb words with one rounding
FLAGS_voxel_classes := -ffp-contract=off
# scan_merge.hip: K9's membership test and K1's binning (regions.h, binning.h) and the interior depth, every fp64 operation rounded once
FLAGS_scan_merge := -ffp-contract=off
# knn.hip: a squared distance is (dx*dx + dy*dy) + dz*dz and a mean a sum of square roots over a count, every fp64 operation rounded once
FLAGS_knn := -ffp-contract=off
# shape.hip: K21's candidate test, a fixed-point offset rint(fl(q - p) * inv), and a covariance and a Jacobi solver whose fp64 operations are rounded once each
FLAGS_shape := -ffp-contract=off
# render.hip: a projected coordinate is ((a0*x + a1*y) + a2*z) + a3 with every product and sum rounded once, as numpy rounds them
FLAGS_render := -ffp-contract=off
# voxel_pool.hip: bins with K1's fp64 rounding sequence (binning.h); a quantum is rint(fl(p - lo) * inv) and a mean lo + (S / n) * step, every fp64 operation rounded once
FLAGS_voxel_pool := -ffp-contract=off

SOURCES := cabi bank voxel conv conv_i8 conv_i8s conv_lin backward corr loss metrics ingest towers crops dbscan tower_score las kitti las_write voxel_cloud thin voxel_classes scan_merge quantile knn shape render voxel_pool
OBJS    := $(SOURCES:%=$(OBJDIR)/%.o)

all: $(OUT)/libscenenet_hip.so

$(OBJDIR)/%.o: $(SRC)/%.hip include/scenenet_hip.h $(wildcard $(SRC)/*.inc) $(wildcard $(SRC)/*.h)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(CXXFLAGS) $(FLAGS_$*) -c $< -o $@

$(OUT)/libscenenet_hip.so: $(OBJS)
	@mkdir -p $(OUT)
	$(HIPCC) -shared -fPIC --offload-arch=$(ARCH) $(OBJS) -o $@

asm: $(SOURCES:%=build/asm/%.s)

build/asm/%.s: $(SRC)/%.hip include/scenenet_hip.h $(wildcard $(SRC)/*.inc) $(wildcard $(SRC)/*.h)
	@mkdir -p build/asm
	$(HIPCC) $(CXXFLAGS) $(FLAGS_$*) -S --cuda-device-only -Rpass-analysis=kernel-resource-usage $< -o $@ \
	  2> build/asm/$*.usage.txt

clean:
	rm -rf build $(OUT)

.PHONY: all asm clean
