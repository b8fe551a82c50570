# Top-level build for C/C++ users (the Python entry point __graft_entry__.build() does the same).
#   make            libmdct_hip.so + the C++ CLI + the CPU checker
#   make lib | cli | jpeg_example | jpegcoef | jpegprog | jpegdec_prog | jpegdec_batch | jpegenc_batch | oracle | ref | clean
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

all: lib cli oracle

# every header is a dependency of every library: no list kept by hand, none to go stale (rebuilding everything takes under a minute)
HEADERS := $(wildcard $(CSRC)/*.h) $(wildcard include/*.h)

lib: $(LIB)
$(LIB): $(CSRC)/mdct_kernels.hip $(CSRC)/mdct_api.hip $(CSRC)/shim.hip $(CSRC)/comm.hip $(CSRC)/stages.hip $(HEADERS)
	$(HIPCC) $(HIPFLAGS) -shared $(CSRC)/mdct_kernels.hip $(CSRC)/mdct_api.hip $(CSRC)/shim.hip $(CSRC)/comm.hip $(CSRC)/stages.hip -ldl -o $@

cli: tools/simd_dct_cli
tools/simd_dct_cli: tools/simd_dct_cli.cpp tools/node_pipeline.h $(LIB)
	$(HIPCC) -O2 -std=c++17 -x hip --offload-arch=$(ARCH) -Iinclude -Itools $< -Lsimd_dct_amd -lmdct_hip -Wl,-rpath,'$$ORIGIN/../simd_dct_amd' -o $@

# plain C on the C-ABI: pixels -> baseline JPEG (tools/mdct_jpeg.c)
jpeg_example: tools/mdct_jpeg
# (no dependency on $(LIB): a GPU test builds this while the library is loaded, so it must never relink it as a side effect; run `make lib` first)
tools/mdct_jpeg: tools/mdct_jpeg.c include/mdct.h
	gcc -O2 -std=c99 -Wall -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude $< -Lsimd_dct_amd -lmdct_hip -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,'$$ORIGIN/../simd_dct_amd' -Wl,-rpath,/opt/rocm/lib -o $@

# JPEG in the coefficient domain (include/mdct_jpegcoef.h), with the library of the table-taking coders it links against; the other JPEG
# stages are built by __graft_entry__.build() (its JPEG_LIBS table)
jpegcoef: simd_dct_amd/libmdct_jpegcoef.so
simd_dct_amd/libmdct_jpegenc_opt.so: $(CSRC)/jpeg_encode_opt.hip $(HEADERS) $(LIB)
	$(HIPCC) $(HIPFLAGS) -shared $< -ldl -Lsimd_dct_amd -lmdct_hip -Wl,-rpath,'$$ORIGIN' -o $@
simd_dct_amd/libmdct_jpegcoef.so: $(CSRC)/jpeg_coef.hip $(HEADERS) simd_dct_amd/libmdct_jpegenc_opt.so
	$(HIPCC) $(HIPFLAGS) -shared $< -ldl -Lsimd_dct_amd -lmdct_jpegenc_opt -lmdct_hip -Wl,-rpath,'$$ORIGIN' -o $@

# the scans of a progressive file from coefficient planes (include/mdct_jpegprog.h)
jpegprog: simd_dct_amd/libmdct_jpegprog.so
simd_dct_amd/libmdct_jpegprog.so: $(CSRC)/jpeg_progressive.hip $(HEADERS) simd_dct_amd/libmdct_jpegenc_opt.so
	$(HIPCC) $(HIPFLAGS) -shared $< -ldl -Lsimd_dct_amd -lmdct_jpegenc_opt -lmdct_hip -Wl,-rpath,'$$ORIGIN' -o $@

# the decoder of a progressive file's scans (include/mdct_jpegdec_prog.h), with the decoder library whose handle and index it takes
jpegdec_prog: simd_dct_amd/libmdct_jpegdec_prog.so
simd_dct_amd/libmdct_jpegdec.so: $(CSRC)/jpeg_decode.hip $(HEADERS) $(LIB)
	$(HIPCC) $(HIPFLAGS) -shared $< -ldl -Lsimd_dct_amd -lmdct_hip -Wl,-rpath,'$$ORIGIN' -o $@
simd_dct_amd/libmdct_jpegdec_prog.so: $(CSRC)/jpeg_decode_progressive.hip $(HEADERS) simd_dct_amd/libmdct_jpegdec.so
	$(HIPCC) $(HIPFLAGS) -shared $< -ldl -Lsimd_dct_amd -lmdct_jpegdec -lmdct_hip -Wl,-rpath,'$$ORIGIN' -o $@

# the restart-marked scans of many files in four launches (include/mdct_jpegdec_batch.h)
jpegdec_batch: simd_dct_amd/libmdct_jpegdec_batch.so
simd_dct_amd/libmdct_jpegdec_batch.so: $(CSRC)/jpeg_decode_batch.hip $(HEADERS) $(LIB)
	$(HIPCC) $(HIPFLAGS) -shared $< -ldl -Lsimd_dct_amd -lmdct_hip -Wl,-rpath,'$$ORIGIN' -o $@

# many RGB images -> their interleaved scans in three launches (include/mdct_jpegenc_batch.h)
jpegenc_batch: simd_dct_amd/libmdct_jpegenc_batch.so
simd_dct_amd/libmdct_jpegenc_batch.so: $(CSRC)/jpeg_encode_batch.hip $(HEADERS) $(LIB)
	$(HIPCC) $(HIPFLAGS) -shared $< -ldl -Lsimd_dct_amd -lmdct_hip -Wl,-rpath,'$$ORIGIN' -o $@

oracle:
	$(MAKE) -C oracle
ref:
	$(MAKE) -C oracle ref

clean:
	rm -f $(LIB) tools/simd_dct_cli tools/mdct_jpeg
	$(MAKE) -C oracle clean

.PHONY: all lib cli jpeg_example jpegcoef jpegprog jpegdec_prog jpegdec_batch jpegenc_batch oracle ref clean
