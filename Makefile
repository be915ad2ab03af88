# Top-level build for C/C++ users (the Python entry point __graft_entry__.build() does the same).
#   make            libgbp_mi355x.so (HIP kernels + C-ABI + host helpers, gfx950), libgbp_mi355x_post.so (the solution readout),
#                   libgbp_mi355x_seed.so (landmark / keyframe seeding), libgbp_mi355x_resect.so (camera resection), libgbp_mi355x_locate.so (camera location) and bin/ba,
#                   bin/slam, bin/bal_convert
#   make oracle     the CPU oracle (test infrastructure)
#   make test       CPU test suite
HIPCC   ?= hipcc
CXX     ?= g++
ARCH    ?= gfx950
PKG     := gbp_poplar_amd
CSRC    := $(PKG)/csrc
LIB     := $(PKG)/libgbp_mi355x.so
# the libraries without a ctx (post: the solution readout, seed: landmark / keyframe seeding, resect: camera resection, locate: camera location with no pose guess): directory $(PKG)/<name>, one rule below
SATELLITES := post seed resect locate
SAT_LIBS := $(SATELLITES:%=$(PKG)/libgbp_mi355x_%.so)
HIPFLAGS := -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden -Wall -Wno-unused-function
OBJDIR  := $(PKG)/_obj/make
# the ROCm tree of $(HIPCC): its headers for the plain C++ translation units, its runtime for the CLIs (--cov_file and --lmk_init hand device arrays to the readout and the seeding)
ROCM    := $(patsubst %/,%,$(dir $(shell readlink -f $$(which $(HIPCC)))))/..
# device code: host + gfx950 pass; the C-ABI (gbp_api_*.cpp, see gbp_ctx.hpp), the device order, the transports, the host helpers: plain C++
# (the rule of gbp_poplar_amd/build.py: every csrc/*.cpp that is not the main of a CLI)
HOST_SRCS := $(filter-out %_main.cpp,$(notdir $(wildcard $(CSRC)/*.cpp)))
OBJS    := $(OBJDIR)/gbp_kernels.o $(HOST_SRCS:%.cpp=$(OBJDIR)/%.o)
# every file under csrc/ that is not itself a compiled translation unit (a csrc/*.cpp, gbp_kernels.hip): headers, the kernel units,
# hooks and experiments that gbp_kernels.hip #includes, the export map
HDRS    := $(filter-out $(CSRC)/gbp_kernels.hip $(wildcard $(CSRC)/*.cpp),$(wildcard $(CSRC)/*.* $(CSRC)/*/*)) $(wildcard include/*.h)

all: $(LIB) $(SAT_LIBS) $(PKG)/bin/ba $(PKG)/bin/slam $(PKG)/bin/bal_convert

$(OBJDIR)/gbp_kernels.o: $(CSRC)/gbp_kernels.hip $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) -c -o $@ $(HIPFLAGS) --offload-arch=$(ARCH) -x hip $<

$(OBJDIR)/%.o: $(CSRC)/%.cpp $(HDRS)
	@mkdir -p $(OBJDIR)
	$(HIPCC) -c -o $@ $(HIPFLAGS) -x c++ -D__HIP_PLATFORM_AMD__ -I$(dir $(shell readlink -f $$(which $(HIPCC))))../include $<

$(LIB): $(OBJS)
	$(HIPCC) -shared -o $@ --offload-arch=$(ARCH) $(OBJS) -ldl -pthread -Wl,--version-script=$(CSRC)/gbp_exports.map

# a ctx-less library (include/gbp_mi355x_<name>.h): one HIP translation unit, the product's flags, an export map of its own;
# $(PKG)/stateless/ is what they share
define SATELLITE_RULES
$(OBJDIR)/gbp_$(1).o: $(PKG)/$(1)/gbp_$(1).hip $$(wildcard $(PKG)/$(1)/*.hpp $(PKG)/stateless/*.hpp) $$(HDRS)
	@mkdir -p $$(OBJDIR)
	$$(HIPCC) -c -o $$@ $$(HIPFLAGS) --offload-arch=$$(ARCH) -x hip $$<

$(PKG)/libgbp_mi355x_$(1).so: $(OBJDIR)/gbp_$(1).o $(PKG)/$(1)/gbp_$(1)_exports.map
	$$(HIPCC) -shared -o $$@ --offload-arch=$$(ARCH) $$< -Wl,--version-script=$(PKG)/$(1)/gbp_$(1)_exports.map
endef
$(foreach s,$(SATELLITES),$(eval $(call SATELLITE_RULES,$(s))))
# locate includes the resection's headers: its Graph, filtering and camera_range, the argument checks of a camera-major call
$(OBJDIR)/gbp_locate.o: $(wildcard $(PKG)/resect/*.hpp)

$(PKG)/bin/%: $(CSRC)/%_main.cpp $(CSRC)/cli_common.hpp $(CSRC)/gbp_transport.hpp $(CSRC)/gbp_metric_gather.hpp include/gbp_mi355x.h include/gbp_mi355x_multi.h include/gbp_mi355x_compat.h include/gbp_mi355x_post.h include/gbp_mi355x_seed.h include/gbp_mi355x_resect.h include/gbp_mi355x_locate.h $(LIB) $(SAT_LIBS)
	@mkdir -p $(PKG)/bin
	$(CXX) -o $@ -O2 -std=c++17 -ffp-contract=off -pthread -D__HIP_PLATFORM_AMD__ -I$(ROCM)/include $< -L$(PKG) -lgbp_mi355x -lgbp_mi355x_post -lgbp_mi355x_seed -lgbp_mi355x_resect -lgbp_mi355x_locate \
		-L$(ROCM)/lib -lamdhip64 -Wl,-rpath,$(ROCM)/lib '-Wl,-rpath,$$ORIGIN/..'

oracle:
	$(MAKE) -C oracle
	@if [ -d /root/reference/ba ]; then $(MAKE) -C oracle ref; fi

test: all oracle
	python -m pytest tests -x -q -m "not gpu"

clean:
	rm -rf $(OBJDIR) $(LIB) $(SAT_LIBS) $(PKG)/bin/ba $(PKG)/bin/slam $(PKG)/bin/bal_convert
	$(MAKE) -C oracle clean

.PHONY: all oracle test clean
