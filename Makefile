# Build of the MI355X-native ALLL solver.
#   make            -> alllsatisfiabilitysolver_amd/liballl.so (HIP kernels + C-ABI, gfx950)
#   make cli        -> tools/alll_main (C++ CLI over the SATInstance compatibility headers)
#   make oracle     -> oracle/liboracle.so (test infrastructure)
#   make ref        -> oracle/_ref/ref_probe (needs /root/reference; test infrastructure)
ROCM ?= /opt/rocm
HIPCC ?= $(ROCM)/bin/hipcc
ARCH ?= gfx950
PKG := alllsatisfiabilitysolver_amd
SRC := $(PKG)/csrc
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -Wall -Wno-unused-result \
            -Iinclude -I$(SRC) -I$(ROCM)/include $(EXTRA)
LIB := $(PKG)/liballl.so
OBJS := $(SRC)/alll_kernels.o $(SRC)/alll_stream.o $(SRC)/alll_refrng.o $(SRC)/alll_runtime.o $(SRC)/alll_layout.o $(SRC)/alll_host.o \
        $(SRC)/alll_small.o $(SRC)/alll_batch.o $(SRC)/alll_batch_runtime.o $(SRC)/alll_propagate.o $(SRC)/alll_score.o $(SRC)/alll_probe.o $(SRC)/alll_residual.o \
        $(SRC)/alll_group.o $(SRC)/alll_group_probe.o $(SRC)/alll_group_runtime.o
GROUP_H := $(SRC)/alll_group.h $(SRC)/alll_group_dev.h
PROP_H := $(SRC)/alll_propagate.h
SCORE_H := $(SRC)/alll_score.h
RESID_H := $(SRC)/alll_residual.h
PROBE_H := $(SRC)/alll_probe.h $(SRC)/alll_group_probe.h

all: $(LIB)

$(SRC)/alll_kernels.o: $(SRC)/alll_kernels.hip $(SRC)/alll_internal.h $(SRC)/alll_draws.h $(GROUP_H)
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(SRC)/alll_stream.o: $(SRC)/alll_stream.hip $(SRC)/alll_internal.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(SRC)/alll_refrng.o: $(SRC)/alll_refrng.hip $(SRC)/alll_internal.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(SRC)/alll_runtime.o: $(SRC)/alll_runtime.cpp $(SRC)/alll_layout.h $(SRC)/alll_internal.h $(SRC)/alll_rt_util.h $(GROUP_H) $(PROP_H) $(SCORE_H) $(RESID_H) $(PROBE_H) include/alll.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(SRC)/alll_layout.o: $(SRC)/alll_layout.cpp $(SRC)/alll_layout.h $(SRC)/alll_internal.h include/alll.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(SRC)/alll_host.o: $(SRC)/alll_host.cpp $(SRC)/alll_draws.h include/alll.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# unit propagation of the pinned variables: the three kernels and their host driver
$(SRC)/alll_propagate.o: $(SRC)/alll_propagate.hip $(PROP_H) $(SRC)/alll_group.h $(SRC)/alll_internal.h $(SRC)/alll_rt_util.h include/alll.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# split scores of the free variables: the scoring kernels and their host driver
$(SRC)/alll_score.o: $(SRC)/alll_score.hip $(SCORE_H) $(PROP_H) $(SRC)/alll_group.h $(SRC)/alll_internal.h $(SRC)/alll_rt_util.h include/alll.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# failed-literal probing: 64 propagations per clause pass, the kernels and their host driver
$(SRC)/alll_probe.o: $(SRC)/alll_probe.hip $(PROBE_H) $(PROP_H) $(SRC)/alll_group.h $(SRC)/alll_internal.h $(SRC)/alll_rt_util.h include/alll.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# the residual formula under the pins: the compaction kernels and their host driver
$(SRC)/alll_residual.o: $(SRC)/alll_residual.hip $(RESID_H) $(PROP_H) $(SRC)/alll_group.h $(SRC)/alll_internal.h $(SRC)/alll_rt_util.h include/alll.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# batches of LDS-resident instances: kernel, host-only planner, device set-up
# (SMALL_REMARKS=-Rpass-analysis=kernel-resource-usage prints the registers, scratch and LDS of both
# instantiations of the batch kernel: DESIGN.md §4.6)
$(SRC)/alll_small.o: $(SRC)/alll_small.hip $(SRC)/alll_small.h $(SRC)/alll_batch.h $(SRC)/alll_draws.h include/alll.h
	$(HIPCC) $(HIPFLAGS) $(SMALL_REMARKS) -c -o $@ $<

$(SRC)/alll_batch.o: $(SRC)/alll_batch.cpp $(SRC)/alll_batch.h include/alll.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(SRC)/alll_batch_runtime.o: $(SRC)/alll_batch_runtime.cpp $(SRC)/alll_small.h $(SRC)/alll_batch.h $(SRC)/alll_rt_util.h include/alll.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# block-diagonal groups: host-only planner, device set-up (the kernels are in alll_kernels.hip)
$(SRC)/alll_group.o: $(SRC)/alll_group.cpp $(SRC)/alll_group.h include/alll.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# probing of a whole group: the host-only planner (the kernels are in alll_probe.hip)
$(SRC)/alll_group_probe.o: $(SRC)/alll_group_probe.cpp $(SRC)/alll_group_probe.h $(SRC)/alll_group.h include/alll.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

$(SRC)/alll_group_runtime.o: $(SRC)/alll_group_runtime.cpp $(GROUP_H) $(PROP_H) $(SCORE_H) $(RESID_H) $(PROBE_H) $(SRC)/alll_internal.h $(SRC)/alll_rt_util.h include/alll.h
	$(HIPCC) $(HIPFLAGS) -c -o $@ $<

# (linked to a temporary name and renamed: a tree snapshot taken meanwhile sees the old or the new library)
$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@.tmp $(OBJS) -L$(ROCM)/lib -lrccl -Wl,-rpath,$(ROCM)/lib
	mv -f $@.tmp $@

cli: tools/alll_main

tools/alll_main: tools/alll_main.cpp $(LIB) include/alll_compat/SATInstance.h
	g++ -O2 -std=c++17 -fopenmp -Iinclude/alll_compat -Iinclude -o $@ tools/alll_main.cpp \
	    -L$(PKG) -lalll -Wl,-rpath,'$$ORIGIN/../$(PKG)'

oracle:
	$(MAKE) -C oracle all

ref:
	$(MAKE) -C oracle ref

clean:
	rm -f $(OBJS) $(LIB) tools/alll_main

.PHONY: all cli oracle ref clean
