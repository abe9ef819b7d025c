# mdfx native build: gfx950 HIP kernels (hipcc), host runtime (g++), pybind11 module, CLIs, tests.
#
#   make -j8            -> mpi_cuda_process_amd/lib/libmdfx.so, mpi_cuda_process_amd/_mdfx*.so,
#                          build/bin/{mdfx,mdf,life,mdfx_tests}
#   make clean
#
# Everything is built in-tree so the shared objects travel with the repository snapshot to the GPU
# box (no JIT cache, no site-packages install).

ROCM      ?= /opt/rocm
HIPCC     ?= $(ROCM)/bin/hipcc
CXX_HOST  ?= g++
ARCH      ?= gfx950
PYTHON    ?= python3

PKG       := mpi_cuda_process_amd
LIBDIR    := $(PKG)/lib
OBJ       := build/obj
BIN       := build/bin

PY_INC    := $(shell $(PYTHON) -c "import sysconfig;print(sysconfig.get_paths()['include'])")
PYBIND_INC:= $(shell $(PYTHON) -c "import pybind11;print(pybind11.get_include())")
PY_EXT    := $(shell $(PYTHON) -c "import sysconfig;print(sysconfig.get_config_var('EXT_SUFFIX'))")

COMMON    := -O3 -std=c++17 -fPIC -Icsrc/include -Wall -Wno-unused-function
HIPFLAGS  := $(COMMON) --offload-arch=$(ARCH) -munsafe-fp-atomics
HOSTFLAGS := $(COMMON) -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include -fopenmp

KERNEL_SRC := $(wildcard csrc/kernels/*.hip)
HOST_SRC   := $(wildcard csrc/core/*.cpp) $(wildcard csrc/cpu/*.cpp) $(wildcard csrc/comm/*.cpp) \
              $(wildcard csrc/engine/*.cpp) $(wildcard csrc/io/*.cpp)
KERNEL_OBJ := $(patsubst csrc/%.hip,$(OBJ)/%.o,$(KERNEL_SRC))
HOST_OBJ   := $(patsubst csrc/%.cpp,$(OBJ)/%.o,$(HOST_SRC))
HEADERS    := $(wildcard csrc/include/mdfx/*.hpp) $(wildcard csrc/kernels/*.hpp) $(wildcard csrc/app/*.hpp)

LIB        := $(LIBDIR)/libmdfx.so
PYMOD      := $(PKG)/_mdfx$(PY_EXT)
APPS       := $(BIN)/mdfx $(BIN)/mdf $(BIN)/life
TESTS      := $(BIN)/mdfx_tests

LINK_ROCM  := -L$(ROCM)/lib -lamdhip64 -lrccl -lgomp -lpthread -ldl

.PHONY: all lib pymod apps tests asan devcheck micro clean
# the default build (and __graft_entry__.build()) is what the GPU runs load; the sanitizer and
# device-check test binaries are separate targets: `make asan devcheck`
all: lib pymod apps tests

lib: $(LIB)
pymod: $(PYMOD)
apps: $(APPS)
tests: $(TESTS)

$(OBJ)/%.o: csrc/%.hip $(HEADERS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(OBJ)/%.o: csrc/%.cpp $(HEADERS)
	@mkdir -p $(dir $@)
	$(CXX_HOST) $(HOSTFLAGS) -c $< -o $@

# the natural-layout rows (heat7_wtk, jacobi5_tbk, box27_tb2n) need the scalar x adds left unpacked (RowOpsN, rowops.hpp)
$(OBJ)/kernels/stencil_heat_wtk.o $(ASAN_DIR)/kernels/stencil_heat_wtk.o $(DCK_DIR)/kernels/stencil_heat_wtk.o: HIPFLAGS += -fno-slp-vectorize
$(OBJ)/kernels/stencil_heat_wxk.o $(ASAN_DIR)/kernels/stencil_heat_wxk.o $(DCK_DIR)/kernels/stencil_heat_wxk.o: HIPFLAGS += -fno-slp-vectorize
$(OBJ)/kernels/stencil_box27_wxk.o $(ASAN_DIR)/kernels/stencil_box27_wxk.o $(DCK_DIR)/kernels/stencil_box27_wxk.o: HIPFLAGS += -fno-slp-vectorize
$(OBJ)/kernels/stencil_heat_tb.o $(ASAN_DIR)/kernels/stencil_heat_tb.o $(DCK_DIR)/kernels/stencil_heat_tb.o: HIPFLAGS += -fno-slp-vectorize
$(OBJ)/kernels/stencil_box27.o $(ASAN_DIR)/kernels/stencil_box27.o $(DCK_DIR)/kernels/stencil_box27.o: HIPFLAGS += -fno-slp-vectorize
# box9 keeps its fp32 arithmetic in plain (unpacked) VALU ops
$(OBJ)/kernels/stencil_box9.o $(ASAN_DIR)/kernels/stencil_box9.o $(DCK_DIR)/kernels/stencil_box9.o: HIPFLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops
$(OBJ)/kernels/stencil_life_rule.o $(ASAN_DIR)/kernels/stencil_life_rule.o $(DCK_DIR)/kernels/stencil_life_rule.o: HIPFLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops
# star7 is one multiply and six fmas per cell, kept in plain (unpacked) VALU ops as well
$(OBJ)/kernels/stencil_star7.o $(ASAN_DIR)/kernels/stencil_star7.o $(DCK_DIR)/kernels/stencil_star7.o: HIPFLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops
# conv9's nine scalar-register weights feed plain (unpacked) VALU multiplies and fmas
$(OBJ)/kernels/stencil_conv9.o $(ASAN_DIR)/kernels/stencil_conv9.o $(DCK_DIR)/kernels/stencil_conv9.o: HIPFLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops
# star13 is one multiply and twelve fmas per cell with three scalar-register weights, plain VALU ops too
$(OBJ)/kernels/stencil_star13.o $(ASAN_DIR)/kernels/stencil_star13.o $(DCK_DIR)/kernels/stencil_star13.o: HIPFLAGS += -Xclang -target-feature -Xclang -packed-fp32-ops

# the AVX2 + FMA copy of the CPU stencils (selected at run time by cpu_kernels.cpp)
$(OBJ)/cpu/cpu_kernels_avx2.o $(ASAN_DIR)/cpu/cpu_kernels_avx2.o $(DCK_DIR)/cpu/cpu_kernels_avx2.o: HOSTFLAGS += -mavx2 -mfma
$(OBJ)/cpu/cpu_kernels.o $(OBJ)/cpu/cpu_kernels_avx2.o: csrc/cpu/cpu_stencils.inc

$(LIB): $(KERNEL_OBJ) $(HOST_OBJ)
	@mkdir -p $(LIBDIR)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $^ $(LINK_ROCM) -Wl,-soname,libmdfx.so -Wl,-rpath,$(ROCM)/lib

$(PYMOD): csrc/python/bindings.cpp $(LIB) $(HEADERS)
	$(CXX_HOST) $(HOSTFLAGS) -fvisibility=hidden -I$(PY_INC) -I$(PYBIND_INC) -shared -o $@ $< \
	  -L$(LIBDIR) -lmdfx -Wl,-rpath,'$$ORIGIN/lib'

$(OBJ)/app/%.o: csrc/app/%.cpp $(HEADERS)
	@mkdir -p $(dir $@)
	$(CXX_HOST) $(HOSTFLAGS) -c $< -o $@

$(BIN)/%: $(OBJ)/app/%_main.o $(OBJ)/app/cli_common.o $(LIB)
	@mkdir -p $(BIN)
	$(CXX_HOST) -o $@ $< $(OBJ)/app/cli_common.o -L$(LIBDIR) -lmdfx $(LINK_ROCM) \
	  -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)' -Wl,-rpath,$(ROCM)/lib

$(TESTS): csrc/tests/test_main.cpp $(LIB) $(HEADERS)
	@mkdir -p $(BIN)
	$(CXX_HOST) $(HOSTFLAGS) -o $@ $< -L$(LIBDIR) -lmdfx $(LINK_ROCM) \
	  -Wl,-rpath,'$$ORIGIN/../../$(LIBDIR)' -Wl,-rpath,$(ROCM)/lib

# Host AddressSanitizer + UBSan build of the native tests (host code only: GPU sanitizers are not
# available on the MI355X pool; on hipcc lines every -fsanitize= follows -Xarch_host).
ASAN_DIR   := build/asan
ASAN_HOST  := -fsanitize=address -fsanitize=undefined -fno-omit-frame-pointer -g
ASAN_HIP   := -Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-omit-frame-pointer
ASAN_KOBJ  := $(patsubst csrc/%.hip,$(ASAN_DIR)/%.o,$(KERNEL_SRC))
ASAN_HOBJ  := $(patsubst csrc/%.cpp,$(ASAN_DIR)/%.o,$(HOST_SRC))
asan: $(BIN)/mdfx_tests_asan

$(ASAN_DIR)/%.o: csrc/%.hip $(HEADERS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) $(ASAN_HIP) -O1 -c $< -o $@

$(ASAN_DIR)/%.o: csrc/%.cpp $(HEADERS)
	@mkdir -p $(dir $@)
	$(CXX_HOST) $(HOSTFLAGS) $(ASAN_HOST) -O1 -c $< -o $@

$(BIN)/mdfx_tests_asan: $(ASAN_DIR)/tests/test_main.o $(ASAN_KOBJ) $(ASAN_HOBJ)
	@mkdir -p $(BIN)
	$(CXX_HOST) $(ASAN_HOST) -o $@ $^ $(LINK_ROCM) -fopenmp -Wl,-rpath,$(ROCM)/lib

# Device-check build of the native tests: every tuned-kernel load / store checks its range against
# the allocation and counts violations (csrc/kernels/kcommon.hpp dcheck); run on a GPU.
DCK_DIR    := build/devcheck
DCK_KOBJ   := $(patsubst csrc/%.hip,$(DCK_DIR)/%.o,$(KERNEL_SRC))
DCK_HOBJ   := $(patsubst csrc/%.cpp,$(DCK_DIR)/%.o,$(HOST_SRC))
devcheck: $(BIN)/mdfx_tests_devcheck

$(DCK_DIR)/%.o: csrc/%.hip $(HEADERS)
	@mkdir -p $(dir $@)
	$(HIPCC) $(HIPFLAGS) -DMDFX_DEVICE_CHECKS -c $< -o $@

$(DCK_DIR)/%.o: csrc/%.cpp $(HEADERS)
	@mkdir -p $(dir $@)
	$(CXX_HOST) $(HOSTFLAGS) -DMDFX_DEVICE_CHECKS -c $< -o $@

$(BIN)/mdfx_tests_devcheck: $(DCK_DIR)/tests/test_main.o $(DCK_KOBJ) $(DCK_HOBJ)
	@mkdir -p $(BIN)
	$(HIPCC) --offload-arch=$(ARCH) -o $@ $^ $(LINK_ROCM) -fopenmp -Wl,-rpath,$(ROCM)/lib

# kernel-variant micro-benchmark (A/B scratch, not part of the engine): make micro
micro: $(BIN)/s7v $(BIN)/copy_roof
$(BIN)/s7v: bench/micro/stencil7_variants.hip
	@mkdir -p $(BIN)
	$(HIPCC) $(HIPFLAGS) -o $@ $<
$(BIN)/copy_roof: bench/micro/copy_roof.hip
	@mkdir -p $(BIN)
	$(HIPCC) $(HIPFLAGS) -o $@ $<

clean:
	rm -rf build $(LIB) $(PYMOD)
