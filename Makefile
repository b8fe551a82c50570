# The one build recipe (the Python entry point __graft_entry__.build() runs it).
#   make            libmdct_hip.so + the twelve JPEG libraries + the C++ CLI + the CPU checker
#   make lib | jpeg | cli | jpeg_example | device-objects | oracle | ref | clean, and one JPEG library by its name: jpegdec, jpegcoef, ...
HIPCC   ?= /opt/rocm/bin/hipcc
ARCH    ?= gfx950
CSRC    := simd_dct_amd/csrc
LIB     := simd_dct_amd/libmdct_hip.so
# -ffp-contract=off: bit-exactness contract (no FMA).  -fno-slp-vectorize: the SLP vectoriser packs adjacent scalar ops
# with v_mov shuffles; where packing pays (the q32 butterflies) it is written by hand.
# -mllvm -disable-vector-combine: LLVM's VectorCombine rewrites a scalar float op on elements of a register pair as a PACKED op with one
# useless half plus a v_mov (twice the issue cycles of the scalar op): the AAN row passes keep 6 / 12 unpaired scalar operations per line
# on purpose (fused int16 round trip 1024 -> 952 vector instructions per wave, 752 -> 632 of them packed).
HIPFLAGS := --offload-arch=$(ARCH) -O3 -ffp-contract=off -fno-slp-vectorize -mllvm -disable-vector-combine -std=c++17 -fPIC -Wall -Iinclude -I$(CSRC)

all: lib jpeg cli oracle

# every header is a dependency of every library: no list kept by hand, none to go stale (rebuilding everything takes under a minute)
HEADERS := $(wildcard $(CSRC)/*.h) $(wildcard include/*.h)

lib: $(LIB)
$(LIB): $(CSRC)/mdct_kernels.hip $(CSRC)/mdct_api.hip $(CSRC)/shim.hip $(CSRC)/comm.hip $(CSRC)/stages.hip $(HEADERS)
	$(HIPCC) $(HIPFLAGS) -shared $(CSRC)/mdct_kernels.hip $(CSRC)/mdct_api.hip $(CSRC)/shim.hip $(CSRC)/comm.hip $(CSRC)/stages.hip -ldl -o $@

cli: tools/simd_dct_cli
tools/simd_dct_cli: tools/simd_dct_cli.cpp tools/node_pipeline.h $(LIB)
	$(HIPCC) -O2 -std=c++17 -x hip --offload-arch=$(ARCH) -Iinclude $< -Lsimd_dct_amd -lmdct_hip -Wl,-rpath,'$$ORIGIN/../simd_dct_amd' -o $@

# plain C on the C-ABI: pixels -> baseline JPEG (tools/mdct_jpeg.c)
jpeg_example: tools/mdct_jpeg
# (no dependency on $(LIB): a GPU test builds this while the library is loaded, so it must never relink it as a side effect; run `make lib` first)
tools/mdct_jpeg: tools/mdct_jpeg.c include/mdct.h
	gcc -O2 -std=c99 -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude $< -Lsimd_dct_amd -lmdct_hip -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../simd_dct_amd' -Wl,-rpath,/opt/rocm/lib -o $@

# The JPEG stages, each its own library linked against libmdct_hip.so, in dependency order:
#   library : source : libraries it links against besides libmdct_hip.so
# (simd_dct_amd/_<library without mdct_>_lib.py binds it and names the same libraries in `after`; tests/test_bindings.py compares)
JPEG_ROWS += mdct_jpegdec:jpeg_decode.hip:  # the decoder of restart-marked scans (include/mdct_jpegdec.h)
JPEG_ROWS += mdct_jpegdec_unmarked:jpeg_decode_unmarked.hip:mdct_jpegdec  # ... of scans without markers
JPEG_ROWS += mdct_jpegdec_prog:jpeg_decode_progressive.hip:mdct_jpegdec  # ... of a progressive file's scans (spectral selection, successive approximation)
JPEG_ROWS += mdct_jpegdec_batch:jpeg_decode_batch.hip:  # ... of the restart-marked scans of many files, four launches in all
JPEG_ROWS += mdct_jpegcolor:jpeg_color.hip:  # chroma upsampling, YCbCr -> RGB
JPEG_ROWS += mdct_jpegscale:jpeg_idct_scaled.hip:  # the inverse at 1/2, 1/4, 1/8 size
JPEG_ROWS += mdct_jpegenc:jpeg_encode_color.hip:  # RGB -> YCbCr, downsampling, padding
JPEG_ROWS += mdct_jpegenc_scan:jpeg_encode_scan.hip:  # three planes -> the Huffman segments of one interleaved scan
JPEG_ROWS += mdct_jpegenc_batch:jpeg_encode_batch.hip:  # many RGB images -> their interleaved scans, three launches in all
JPEG_ROWS += mdct_jpegenc_opt:jpeg_encode_opt.hip:  # symbol statistics, optimal tables, coders that take them
JPEG_ROWS += mdct_jpegcoef:jpeg_coef.hip:mdct_jpegenc_opt  # coefficient planes -> segments; flips, transposes, rotations
JPEG_ROWS += mdct_jpegprog:jpeg_progressive.hip:mdct_jpegenc_opt  # coefficient planes -> the scans of a progressive file

# $(call JPEG_RULE,library,source,links): the library's rule and its short target (mdct_jpegcoef -> jpegcoef); a library it links
# against stands for $(LIB) as a dependency, being newer
define JPEG_RULE
$(1:mdct_%=%): simd_dct_amd/lib$(1).so
simd_dct_amd/lib$(1).so: $$(CSRC)/$(2) $$(HEADERS) $(if $(3),$(3:%=simd_dct_amd/lib%.so),$$(LIB))
	$$(HIPCC) $$(HIPFLAGS) -shared $$< -ldl -Lsimd_dct_amd $(patsubst %,-l%,$(3) mdct_hip) -Wl,-rpath,'$$$$ORIGIN' -o $$@
endef
row = $(word $(1),$(subst :, ,$(2)))
$(foreach r,$(JPEG_ROWS),$(eval $(call JPEG_RULE,$(call row,1,$(r)),$(call row,2,$(r)),$(call row,3,$(r)))))
JPEG_NAMES := $(foreach r,$(JPEG_ROWS),$(call row,1,$(r)))
jpeg: $(JPEG_NAMES:mdct_%=%)

# the device object of every translation unit, as DESIGN.md section 9 lists their hashes: the library flags, device side only.  The
# command line enters the object, so the hashes hold for this command alone: from this directory, relative paths, into _dv/
device-objects:
	@mkdir -p _dv
	@for f in $(sort $(wildcard $(CSRC)/*.hip)); do $(HIPCC) $(HIPFLAGS) --cuda-device-only -c $$f -o _dv/$$(basename $$f .hip).o || exit 1; done
	@sha256sum _dv/*.o

oracle:
	$(MAKE) -C oracle
ref:
	$(MAKE) -C oracle ref

clean:
	rm -f $(LIB) $(JPEG_NAMES:%=simd_dct_amd/lib%.so) tools/simd_dct_cli tools/mdct_jpeg
	$(MAKE) -C oracle clean

.PHONY: all lib cli jpeg_example jpeg $(JPEG_NAMES:mdct_%=%) device-objects oracle ref clean
