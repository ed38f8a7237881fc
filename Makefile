# Build of the MI355X raycaster (gfx950) — everything in-tree.
#
#   make            libraycast_hip.so (HIP kernels + C-ABI), libraycast_front.so (host
#                   scene parser / P3 writer), bin/raytrace (drop-in CLI), oracle, primcheck
#                   (tests/build/libprimcheck.so, the ray-level suite's device harness), pincheck
#                   (tests/build/libpincheck.so, phase C's carry-point table wave by wave), resolvecheck
#                   (tests/build/libresolvecheck.so and its four wrong variants, the carry resolver
#                   entry by entry), compactcheck (tests/build/libcompactcheck.so and its five wrong
#                   variants, the DEP compaction and the row-shard kernels class map by class map), listcheck
#                   (tests/build/liblistcheck.so and its eight wrong variants, the edge list and the
#                   rate binning plane by plane)
#   make ref        oracle/_ref: the reference C/ sources compiled in place (test oracle)
#
# Numerics flags (parity with the x86-64 gcc -O3 reference):
#   -ffp-contract=off                    no a*b+c fusion (hipcc defaults to fast-honor-pragmas)
#   -fno-gpu-flush-denormals-to-zero     f32 denormals kept, like SSE2
#   -fhip-fp32-correctly-rounded-divide-sqrt   IEEE f32 division
# Host C: gcc -O3 without -march (no FMA), like C/Makefile:4.

HIPCC   ?= /opt/rocm/bin/hipcc
CC      ?= gcc
PKG     := raytracing-programs_amd
SRC     := $(PKG)/csrc
LIB     := $(PKG)/lib
BIN     := $(PKG)/bin
OBJ     := $(PKG)/lib/obj
ARCH    ?= gfx950

HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off \
            -fno-gpu-flush-denormals-to-zero -fhip-fp32-correctly-rounded-divide-sqrt \
            -Iinclude -I$(SRC) -Wall -Wno-gnu-anonymous-struct -Wno-nested-anon-types \
            -Wno-c11-extensions -Wno-unused-result
CFLAGS   := -O3 -ffp-contract=off -fPIC -Wall -Wno-unused-result -Iinclude -I$(SRC)

HIP_SRCS  := $(SRC)/rc_kernels.hip $(SRC)/rc_sample_kernels.hip $(SRC)/rc_api.hip $(SRC)/rc_sampling.hip $(SRC)/rc_shard.hip $(SRC)/rc_filter.hip $(SRC)/rc_guided.hip
HIP_HDRS  := $(SRC)/rc_device.hpp $(SRC)/rc_cudasem.hpp $(SRC)/rc_pixel.hpp $(SRC)/rc_resolve.hpp $(SRC)/rc_compact.hpp $(SRC)/rc_lists.hpp $(SRC)/rc_rates_bin.inc $(SRC)/rc_kernels.h $(SRC)/rc_runtime.h $(SRC)/rc_scene.h include/raycast_hip.h
FRONT_SRC := $(SRC)/front/parse.c $(SRC)/front/objects.c $(SRC)/front/ppm.c

.PHONY: all oracle ref clean stamps stamps2 sanitize primcheck pincheck resolvecheck compactcheck listcheck
all: $(LIB)/libraycast_hip.so $(LIB)/libraycast_front.so $(BIN)/raytrace oracle primcheck pincheck resolvecheck compactcheck listcheck

$(OBJ)/%.o: $(SRC)/%.hip $(HIP_HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJ)/rc_scene.o: $(SRC)/rc_scene.c $(SRC)/rc_scene.h include/raycast_hip.h
	@mkdir -p $(OBJ)
	$(CC) $(CFLAGS) -c $< -o $@

ROCM    ?= /opt/rocm
HIPLIBS := -L$(ROCM)/lib -lrccl -Wl,-rpath,$(ROCM)/lib -lpthread
# the objects every variant of the library shares with the product: they are built without the
# variants' -D options (RC_STAMPS and RC_DIAG reach rc_kernels.hip and rc_api.hip only, the kernels'
# -D options rc_kernels.hip only: the render, parity and phase C kernels), so the sampling kernels
# of every variant are the product's
PLAIN_OBJS := $(OBJ)/rc_sample_kernels.o $(OBJ)/rc_sampling.o $(OBJ)/rc_shard.o $(OBJ)/rc_filter.o $(OBJ)/rc_guided.o $(OBJ)/rc_scene.o

$(LIB)/libraycast_hip.so: $(OBJ)/rc_kernels.o $(OBJ)/rc_api.o $(PLAIN_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@ $(HIPLIBS)

$(LIB)/libraycast_front.so: $(FRONT_SRC) include/raycast_hip.h
	@mkdir -p $(LIB)
	$(CC) $(CFLAGS) -shared $(FRONT_SRC) -o $@ -lm -lpthread

$(BIN)/raytrace: $(SRC)/front/raytrace_main.c $(LIB)/libraycast_front.so $(LIB)/libraycast_hip.so
	@mkdir -p $(BIN)
	$(CC) $(CFLAGS) $< -L$(LIB) -lraycast_front -lraycast_hip -Wl,-rpath,'$$ORIGIN/../lib' -o $@

# diagnostic build with in-kernel cycle stamps and the RC_RESOLVE_TRACE / RC_SIDE_STATS dumps
# (RC_HIP_LIB=libraycast_hip_stamps.so); the product library reads only RAYCAST_* options
stamps: $(LIB)/libraycast_hip_stamps.so
$(OBJ)/stamps_kernels.o: $(SRC)/rc_kernels.hip $(HIP_HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DRC_STAMPS=1 -DRC_DIAG=1 -c $< -o $@
$(OBJ)/stamps_api.o: $(SRC)/rc_api.hip $(HIP_HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DRC_STAMPS=1 -DRC_DIAG=1 -c $< -o $@
$(LIB)/libraycast_hip_stamps.so: $(OBJ)/stamps_kernels.o $(OBJ)/stamps_api.o $(PLAIN_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@ $(HIPLIBS)
# coarse stamps: only per-step cycle counts (the evaluator itself is the product code)
stamps2: $(LIB)/libraycast_hip_stamps2.so
$(OBJ)/stamps2_kernels.o: $(SRC)/rc_kernels.hip $(HIP_HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DRC_STAMPS=2 -DRC_DIAG=1 -c $< -o $@
$(OBJ)/stamps2_api.o: $(SRC)/rc_api.hip $(HIP_HDRS)
	@mkdir -p $(OBJ)
	$(HIPCC) $(HIPFLAGS) -DRC_STAMPS=2 -DRC_DIAG=1 -c $< -o $@
$(LIB)/libraycast_hip_stamps2.so: $(OBJ)/stamps2_kernels.o $(OBJ)/stamps2_api.o $(PLAIN_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@ $(HIPLIBS)

oracle:
	$(MAKE) -C oracle oracle

ref:
	$(MAKE) -C oracle ref

clean:
	rm -rf $(LIB) $(BIN) $(PRIM_OUT)
	$(MAKE) -C oracle clean

# measurement variants of the pixel kernels' framebuffer store (RC_HIP_LIB=libraycast_hip_<v>.so):
#   coalesced: 32x8 tiles staged in LDS, whole-row stores; t16: 16x16 tiles staged in LDS
variants: $(LIB)/libraycast_hip_coalesced.so $(LIB)/libraycast_hip_t16.so
$(OBJ)/coalesced_kernels.o: $(SRC)/rc_kernels.hip $(HIP_HDRS)
	$(HIPCC) $(HIPFLAGS) -DRC_TILE_W=32 -DRC_TILE_STAGE=1 -c $< -o $@
$(OBJ)/t16_kernels.o: $(SRC)/rc_kernels.hip $(HIP_HDRS)
	$(HIPCC) $(HIPFLAGS) -DRC_TILE_W=16 -DRC_TILE_STAGE=1 -c $< -o $@
# occupancy variants of the pixel kernels (RC_PHASE_A_WAVES waves per SIMD)
$(OBJ)/pa5_kernels.o: $(SRC)/rc_kernels.hip $(HIP_HDRS)
	$(HIPCC) $(HIPFLAGS) -DRC_PHASE_A_WAVES=5 -c $< -o $@
$(OBJ)/pa6_kernels.o: $(SRC)/rc_kernels.hip $(HIP_HDRS)
	$(HIPCC) $(HIPFLAGS) -DRC_PHASE_A_WAVES=6 -c $< -o $@
$(LIB)/libraycast_hip_%.so: $(OBJ)/%_kernels.o $(OBJ)/rc_api.o $(PLAIN_OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@ $(HIPLIBS)

# measurement variants of k_camera (scripts/camera_ab.py): the eye's LDS table (camtable) against
# the general nearest with O = eye (camgen); every other kernel of both is the product's
camera-variants: $(LIB)/libraycast_hip_camtable.so $(LIB)/libraycast_hip_camgen.so
$(OBJ)/camtable_sample_kernels.o: $(SRC)/rc_sample_kernels.hip $(HIP_HDRS)
	$(HIPCC) $(HIPFLAGS) -DRC_CAMERA_TABLE=1 -c $< -o $@
$(OBJ)/camgen_sample_kernels.o: $(SRC)/rc_sample_kernels.hip $(HIP_HDRS)
	$(HIPCC) $(HIPFLAGS) -DRC_CAMERA_TABLE=0 -c $< -o $@
$(LIB)/libraycast_hip_cam%.so: $(OBJ)/rc_kernels.o $(OBJ)/rc_api.o $(OBJ)/cam%_sample_kernels.o $(filter-out $(OBJ)/rc_sample_kernels.o,$(PLAIN_OBJS))
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@ $(HIPLIBS)

# measurement variant of k_ao_filter (scripts/ao_filter_ab.py): the neighbours read from global
# memory through the caches (aofdirect) against the product's LDS-staged tile; every other kernel
# is the product's
filter-variants: $(LIB)/libraycast_hip_aofdirect.so
$(OBJ)/aofdirect_guided.o: $(SRC)/rc_guided.hip $(HIP_HDRS)
	$(HIPCC) $(HIPFLAGS) -DRC_AO_FILTER_DIRECT=1 -c $< -o $@
$(LIB)/libraycast_hip_aofdirect.so: $(OBJ)/rc_kernels.o $(OBJ)/rc_api.o $(OBJ)/aofdirect_guided.o $(filter-out $(OBJ)/rc_guided.o,$(PLAIN_OBJS))
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC $^ -o $@ $(HIPLIBS)

# ASan + UBSan builds of the host C (tests/test_sanitize.py; SURVEY.md §5: the CPU restatement
# must not rely on UB): the oracle's CLI and the front end (parse / lists / P3 writer) driven
# by tests/tools/front_check.c.  Host code only; no GPU code is sanitized.
SAN     := -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g
SAN_OUT := build/sanitize
sanitize: $(SAN_OUT)/oracle_raytrace $(SAN_OUT)/front_check
$(SAN_OUT)/oracle_raytrace: oracle/oracle_main.c oracle/rc_oracle.c oracle/rc_oracle.h include/raycast_hip.h
	@mkdir -p $(SAN_OUT)
	$(CC) -O1 -ffp-contract=off $(SAN) -Iinclude oracle/oracle_main.c oracle/rc_oracle.c -o $@ -lm
$(SAN_OUT)/front_check: tests/tools/front_check.c $(FRONT_SRC) include/raycast_hip.h
	@mkdir -p $(SAN_OUT)
	$(CC) -O1 -ffp-contract=off $(SAN) -Iinclude -I$(SRC) tests/tools/front_check.c $(FRONT_SRC) -o $@ -lm -lpthread

# Test-only device harness of the ray-level suite (tests/test_gpu_prims.py): the product's own
# rc_device.hpp / rc_cudasem.hpp routines behind plain C entries, one thread per case, compiled
# with the product's HIPFLAGS and fed by rc_pack_scene's records (rc_scene.o).  The product
# library never links it.
PRIM_OUT := tests/build
primcheck: $(PRIM_OUT)/libprimcheck.so
$(PRIM_OUT)/libprimcheck.so: tests/tools/prim_check.hip $(HIP_HDRS) $(OBJ)/rc_scene.o | oracle
	@mkdir -p $(PRIM_OUT)
	$(HIPCC) $(HIPFLAGS) -shared $(OBJ)/rc_scene.o tests/tools/prim_check.hip -o $@ -Wl,-rpath,$(ROCM)/lib

# Test-only device harness of phase C's carry-point table (tests/test_gpu_pinned.py): one wave per
# 64 entries through the product's shade_dep_wave, built like primcheck.
pincheck: $(PRIM_OUT)/libpincheck.so
$(PRIM_OUT)/libpincheck.so: tests/tools/pin_check.hip $(HIP_HDRS) $(OBJ)/rc_scene.o | oracle
	@mkdir -p $(PRIM_OUT)
	$(HIPCC) $(HIPFLAGS) -shared $(OBJ)/rc_scene.o tests/tools/pin_check.hip -o $@ -Wl,-rpath,$(ROCM)/lib

# Test-only device harness of the carry resolver (tests/test_gpu_resolve.py): the evaluator forms
# case by case and the product's wave_window / block_window (rc_resolve.hpp) chain by chain, built
# like primcheck.  libresolvecheck_w1..w4.so are the same harness with one deliberate mistake each
# (RV_WRONG), which the suite must catch.
RESOLVE_LIBS := $(PRIM_OUT)/libresolvecheck.so $(foreach k,1 2 3 4,$(PRIM_OUT)/libresolvecheck_w$(k).so)
resolvecheck: $(RESOLVE_LIBS)
$(PRIM_OUT)/libresolvecheck.so: tests/tools/resolve_check.hip $(HIP_HDRS) $(OBJ)/rc_scene.o | oracle
	@mkdir -p $(PRIM_OUT)
	$(HIPCC) $(HIPFLAGS) -shared $(OBJ)/rc_scene.o tests/tools/resolve_check.hip -o $@ -Wl,-rpath,$(ROCM)/lib
$(PRIM_OUT)/libresolvecheck_w%.so: tests/tools/resolve_check.hip $(HIP_HDRS) $(OBJ)/rc_scene.o | oracle
	@mkdir -p $(PRIM_OUT)
	$(HIPCC) $(HIPFLAGS) -DRV_WRONG=$* -shared $(OBJ)/rc_scene.o tests/tools/resolve_check.hip -o $@ -Wl,-rpath,$(ROCM)/lib

# Test-only device harness of the DEP compaction and the row shards (tests/test_gpu_compact.py):
# the product's rc_compact.hpp kernels over class maps and segment tables, launched as the
# launchers launch them, built like primcheck (no scene: nothing but the HIP runtime is linked).
# libcompactcheck_w1..w5.so are the same harness with one deliberate mistake each (CV_WRONG),
# which the suite must catch.
COMPACT_LIBS := $(PRIM_OUT)/libcompactcheck.so $(foreach k,1 2 3 4 5,$(PRIM_OUT)/libcompactcheck_w$(k).so)
compactcheck: $(COMPACT_LIBS)
$(PRIM_OUT)/libcompactcheck.so: tests/tools/compact_check.hip $(HIP_HDRS)
	@mkdir -p $(PRIM_OUT)
	$(HIPCC) $(HIPFLAGS) -shared tests/tools/compact_check.hip -o $@ -Wl,-rpath,$(ROCM)/lib
$(PRIM_OUT)/libcompactcheck_w%.so: tests/tools/compact_check.hip $(HIP_HDRS)
	@mkdir -p $(PRIM_OUT)
	$(HIPCC) $(HIPFLAGS) -DCV_WRONG=$* -shared tests/tools/compact_check.hip -o $@ -Wl,-rpath,$(ROCM)/lib

# Test-only device harness of the sampling family's list builders (tests/test_gpu_lists.py): the
# product's rc_lists.hpp and rc_rates_bin.inc (k_aa_mark and the binning block of k_rates_render) over
# planes of bytes, launched as the launchers launch them, built like compactcheck.
# liblistcheck_w1..w8.so are the same harness with one deliberate mistake each (LV_WRONG), which
# the suite must catch.
LIST_LIBS := $(PRIM_OUT)/liblistcheck.so $(foreach k,1 2 3 4 5 6 7 8,$(PRIM_OUT)/liblistcheck_w$(k).so)
listcheck: $(LIST_LIBS)
$(PRIM_OUT)/liblistcheck.so: tests/tools/list_check.hip $(HIP_HDRS)
	@mkdir -p $(PRIM_OUT)
	$(HIPCC) $(HIPFLAGS) -shared tests/tools/list_check.hip -o $@ -Wl,-rpath,$(ROCM)/lib
$(PRIM_OUT)/liblistcheck_w%.so: tests/tools/list_check.hip $(HIP_HDRS)
	@mkdir -p $(PRIM_OUT)
	$(HIPCC) $(HIPFLAGS) -DLV_WRONG=$* -shared tests/tools/list_check.hip -o $@ -Wl,-rpath,$(ROCM)/lib

# occupancy variants of the pixel kernels (RC_HIP_LIB=libraycast_hip_<v>.so): w3 = phase A /
# k_render compiled for 3 waves per SIMD (no VGPR spills), f3 = phase C (k_dep_chunks, k_finish)
occupancy: $(LIB)/libraycast_hip_w3.so $(LIB)/libraycast_hip_f3.so $(LIB)/libraycast_hip_c512.so $(LIB)/libraycast_hip_c2048.so
$(OBJ)/c512_kernels.o: $(SRC)/rc_kernels.hip $(HIP_HDRS)
	$(HIPCC) $(HIPFLAGS) -DRC_CHUNK=512 -c $< -o $@
$(OBJ)/c2048_kernels.o: $(SRC)/rc_kernels.hip $(HIP_HDRS)
	$(HIPCC) $(HIPFLAGS) -DRC_CHUNK=2048 -c $< -o $@
$(OBJ)/w3_kernels.o: $(SRC)/rc_kernels.hip $(HIP_HDRS)
	$(HIPCC) $(HIPFLAGS) -DRC_PHASE_A_WAVES=3 -c $< -o $@
$(OBJ)/f3_kernels.o: $(SRC)/rc_kernels.hip $(HIP_HDRS)
	$(HIPCC) $(HIPFLAGS) -DRC_FINISH_WAVES=3 -c $< -o $@
