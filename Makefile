# Build: the HIP engine (gfx950) and the CPU oracle (test infrastructure only).
HIPCC   ?= /opt/rocm/bin/hipcc
CXX     ?= g++
ARCH    ?= gfx950
JOBS    ?= 8

LIB     := wiser_amd/_lib/libwiser_hip.so
ORACLE  := oracle/_build/liboracle.so
SRCS    := wiser_amd/csrc/writer.cc wiser_amd/csrc/index.cc wiser_amd/csrc/engine.cc \
           wiser_amd/csrc/shard_exchange.cc wiser_amd/csrc/batch_plan.cc wiser_amd/csrc/server.cc \
           wiser_amd/csrc/score_plan.cc wiser_amd/csrc/score_docs.cc \
           wiser_amd/csrc/bool_plan.cc wiser_amd/csrc/bool_run.cc wiser_amd/csrc/bool_search.cc \
           wiser_amd/csrc/count_bool.cc wiser_amd/csrc/docset.cc \
           wiser_amd/csrc/docstore.cc \
           wiser_amd/csrc/snippet.cc wiser_amd/csrc/kernels.hip
HDRS    := $(wildcard wiser_amd/csrc/*.h) include/wiser_hip.h
OBJDIR  := wiser_amd/_lib/obj
OBJS    := $(patsubst wiser_amd/csrc/%,$(OBJDIR)/%.o,$(SRCS))

# -ffp-contract=off everywhere: the reference build has no FMA (CMakeLists.txt:6,12)
HIPFLAGS := --offload-arch=$(ARCH) -O3 -std=c++17 -fPIC -ffp-contract=off -Wall \
            -Wno-unused-function
ORAFLAGS := -O3 -DNDEBUG -std=c++17 -fPIC -ffp-contract=off -Wall -shared

CLI     := wiser_amd/_lib/engine_cli
CALIB   := wiser_amd/_lib/calib_ea
DICT    := wiser_amd/_lib/dict_check
DEVMEM  := wiser_amd/_lib/dev_mem_check
BPLAN   := wiser_amd/_lib/batch_plan_check
TPLAN   := wiser_amd/_lib/tiny_plan_check
SLAYOUT := wiser_amd/_lib/shard_layout_check
SPLAN   := wiser_amd/_lib/score_plan_check
SCLI    := wiser_amd/_lib/score_cli
BLMIMG  := wiser_amd/_lib/bloom_image_check
BOPLAN  := wiser_amd/_lib/bool_plan_check
BOCLI   := wiser_amd/_lib/bool_cli
COPLAN  := wiser_amd/_lib/count_plan_check
COCLI   := wiser_amd/_lib/count_cli
DSCLI   := wiser_amd/_lib/docset_cli

# (the buffer owner's, the two plans' and the shard layout's checks are tests of those files
# alone: a tree whose tests/ does not hold their sources still builds everything else)
all: $(LIB) $(ORACLE) $(CLI) $(CALIB) $(DICT) $(if $(wildcard tests/cpp/dev_mem_check.cc),$(DEVMEM)) \
     $(if $(wildcard tests/cpp/batch_plan_check.cc),$(BPLAN)) \
     $(if $(wildcard tests/cpp/tiny_plan_check.cc),$(TPLAN)) \
     $(if $(wildcard tests/cpp/shard_layout_check.cc),$(SLAYOUT)) \
     $(if $(wildcard tests/cpp/score_plan_check.cc),$(SPLAN)) \
     $(if $(wildcard tests/cpp/score_cli.cc),$(SCLI)) \
     $(if $(wildcard tests/cpp/bloom_image_check.cc),$(BLMIMG)) \
     $(if $(wildcard tests/cpp/bool_plan_check.cc),$(BOPLAN)) \
     $(if $(wildcard tests/cpp/bool_cli.cc),$(BOCLI)) \
     $(if $(wildcard tests/cpp/count_plan_check.cc),$(COPLAN)) \
     $(if $(wildcard tests/cpp/count_cli.cc),$(COCLI)) \
     $(if $(wildcard tests/cpp/docset_cli.cc),$(DSCLI))

# CPU check of the term dictionary (tests/test_dictionary.py)
$(DICT): tests/cpp/dict_check.cc wiser_amd/csrc/index.h $(LIB)
	$(CXX) -O2 -std=c++17 -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -o $@ tests/cpp/dict_check.cc -Lwiser_amd/_lib -lwiser_hip -Wl,-rpath,'$$ORIGIN'

# CPU check of a shard image's bloom filters against the whole image's (tests/test_bloom_image.py)
$(BLMIMG): tests/cpp/bloom_image_check.cc wiser_amd/csrc/index.h wiser_amd/csrc/engine_types.h $(LIB)
	$(CXX) -O2 -std=c++17 -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ -o $@ tests/cpp/bloom_image_check.cc -Lwiser_amd/_lib -lwiser_hip -Wl,-rpath,'$$ORIGIN'

# CPU check of the buffer owner over a fake memory policy (tests/test_dev_mem.py): no HIP, no engine
$(DEVMEM): tests/cpp/dev_mem_check.cc wiser_amd/csrc/dev_mem.h
	@mkdir -p wiser_amd/_lib
	$(CXX) -O2 -std=c++17 -Wall -o $@ tests/cpp/dev_mem_check.cc

# CPU check of the upload plan on a hand-made image (tests/test_batch_plan.py): no HIP, no engine
$(BPLAN): tests/cpp/batch_plan_check.cc wiser_amd/csrc/batch_plan.cc wiser_amd/csrc/batch_plan.h \
          wiser_amd/csrc/or_plan.h \
          wiser_amd/csrc/engine_types.h include/wiser_hip.h
	@mkdir -p wiser_amd/_lib
	$(CXX) -O2 -std=c++17 -Wall -o $@ tests/cpp/batch_plan_check.cc wiser_amd/csrc/batch_plan.cc

# CPU check of the tiny class in the upload plan (tests/test_tiny_plan.py): no HIP, no engine
$(TPLAN): tests/cpp/tiny_plan_check.cc wiser_amd/csrc/batch_plan.cc wiser_amd/csrc/batch_plan.h \
          wiser_amd/csrc/or_plan.h \
          wiser_amd/csrc/engine_types.h include/wiser_hip.h
	@mkdir -p wiser_amd/_lib
	$(CXX) -O2 -std=c++17 -Wall -o $@ tests/cpp/tiny_plan_check.cc wiser_amd/csrc/batch_plan.cc

# CPU check of the shard exchange's region layout and its two device views (tests/test_shard_layout.py):
# no HIP, no engine
$(SLAYOUT): tests/cpp/shard_layout_check.cc wiser_amd/csrc/shard_layout.h wiser_amd/csrc/engine_types.h
	@mkdir -p wiser_amd/_lib
	$(CXX) -O2 -std=c++17 -Wall -o $@ tests/cpp/shard_layout_check.cc

# CPU check of the wsr_score_docs plan on a hand-made image (tests/test_score_plan.py): no HIP, no engine
$(SPLAN): tests/cpp/score_plan_check.cc wiser_amd/csrc/score_plan.cc wiser_amd/csrc/score_plan.h \
          wiser_amd/csrc/batch_plan.h wiser_amd/csrc/engine_types.h include/wiser_hip.h
	@mkdir -p wiser_amd/_lib
	$(CXX) -O2 -std=c++17 -Wall -o $@ tests/cpp/score_plan_check.cc wiser_amd/csrc/score_plan.cc

# CPU check of the wsr_search_bool plan on a hand-made image (tests/test_bool_plan.py): no HIP, no engine
$(BOPLAN): tests/cpp/bool_plan_check.cc wiser_amd/csrc/bool_plan.cc wiser_amd/csrc/bool_plan.h \
           wiser_amd/csrc/or_plan.h wiser_amd/csrc/batch_plan.h wiser_amd/csrc/engine_types.h include/wiser_hip.h
	@mkdir -p wiser_amd/_lib
	$(CXX) -O2 -std=c++17 -Wall -o $@ tests/cpp/bool_plan_check.cc wiser_amd/csrc/bool_plan.cc

# CPU check of the wsr_count_bool plan on a hand-made image (tests/test_count_plan.py): no HIP, no engine
$(COPLAN): tests/cpp/count_plan_check.cc wiser_amd/csrc/bool_plan.cc wiser_amd/csrc/bool_plan.h \
           wiser_amd/csrc/or_plan.h wiser_amd/csrc/batch_plan.h wiser_amd/csrc/engine_types.h include/wiser_hip.h
	@mkdir -p wiser_amd/_lib
	$(CXX) -O2 -std=c++17 -Wall -o $@ tests/cpp/count_plan_check.cc wiser_amd/csrc/bool_plan.cc

# counter calibration (profiles only): known-byte reads for rocprofv3 --pmc
$(CALIB): scripts/calib_ea.hip
	@mkdir -p wiser_amd/_lib
	$(HIPCC) --offload-arch=$(ARCH) -O3 -o $@ $<

$(CLI): tests/cpp/engine_cli.cc include/wiser_hip_engine.hpp include/wiser_hip.h $(LIB)
	$(CXX) -O2 -std=c++17 -Iinclude -o $@ tests/cpp/engine_cli.cc -Lwiser_amd/_lib -lwiser_hip -Wl,-rpath,'$$ORIGIN'

# C++ host of the (query, doc) scoring mirror (tests/test_gpu_score_docs.py)
$(SCLI): tests/cpp/score_cli.cc include/wiser_hip_engine.hpp include/wiser_hip.h $(LIB)
	$(CXX) -O2 -std=c++17 -Iinclude -o $@ tests/cpp/score_cli.cc -Lwiser_amd/_lib -lwiser_hip -Wl,-rpath,'$$ORIGIN'

# C++ host of the boolean query mirror (tests/test_gpu_bool.py)
$(BOCLI): tests/cpp/bool_cli.cc include/wiser_hip_engine.hpp include/wiser_hip.h $(LIB)
	$(CXX) -O2 -std=c++17 -Iinclude -o $@ tests/cpp/bool_cli.cc -Lwiser_amd/_lib -lwiser_hip -Wl,-rpath,'$$ORIGIN'

# C++ host of the match-count mirror (tests/test_gpu_count.py)
$(COCLI): tests/cpp/count_cli.cc include/wiser_hip_engine.hpp include/wiser_hip.h $(LIB)
	$(CXX) -O2 -std=c++17 -Iinclude -o $@ tests/cpp/count_cli.cc -Lwiser_amd/_lib -lwiser_hip -Wl,-rpath,'$$ORIGIN'

# C++ host of the doc-set mirror (tests/test_gpu_docset.py)
$(DSCLI): tests/cpp/docset_cli.cc include/wiser_hip_engine.hpp include/wiser_hip.h $(LIB)
	$(CXX) -O2 -std=c++17 -Iinclude -o $@ tests/cpp/docset_cli.cc -Lwiser_amd/_lib -lwiser_hip -Wl,-rpath,'$$ORIGIN'

$(OBJDIR)/%.o: wiser_amd/csrc/% $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) $(HIPFLAGS) -c $< -o $@

$(LIB): $(OBJS)
	$(HIPCC) --offload-arch=$(ARCH) -shared -fPIC -o $@ $(OBJS) -lpthread -l:liblz4.so.1 -lrccl

$(ORACLE): oracle/oracle.cc oracle/oracle.h
	@mkdir -p oracle/_build
	$(CXX) $(ORAFLAGS) -o $@ oracle/oracle.cc -lpthread -l:liblz4.so.1

clean:
	rm -rf wiser_amd/_lib oracle/_build

.PHONY: all clean
