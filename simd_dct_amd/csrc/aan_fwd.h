// aan_fwd.h -- device pieces of the engine-own FORWARD path that more than one translation unit compiles: the packed-fp32 helpers,
// the quantiser's constants, the 8-byte row load, the byte -> float convert, the constant pairs of the AAN passes and the scalar-load
// views of a kernel's argument segment.  Everything aan_passes.h -- the AAN passes, the quantiser and the zig-zag compaction that
// mdct_kernels.hip (libmdct_hip.so) and the JPEG scan coders (jpeg_encode_scan.hip, jpeg_encode_opt.hip, jpeg_coef.hip: a library each)
// all compile -- and the chunk skeleton of those coders (scan_chunks.h) are written in.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mdct_kernels.h"

#pragma clang fp contract(off)

namespace mdct
{

typedef float f32x2 __attribute__((ext_vector_type(2)));
#define MDCT_PKA(d, a, b, mods) asm("v_pk_add_f32 %0, %1, %2 " mods : "=v"(d) : "v"(a), "v"(b))
#define MDCT_PKM(d, a, k, mods) asm("v_pk_mul_f32 %0, %1, %2 " mods : "=v"(d) : "v"(a), "s"(k))
#define MDCT_PKF(d, a, k, c, mods) asm("v_pk_fma_f32 %0, %1, %2, %3 " mods : "=v"(d) : "v"(a), "s"(k), "v"(c)) // d = a * k + c, one rounding
// halves of the constant operand (src1) used for (lo, hi) of the result
#define MDCT_K_LL "op_sel:[0,0] op_sel_hi:[1,0]"
#define MDCT_K_HH "op_sel:[0,1] op_sel_hi:[1,1]"
#define MDCT_K_LH "op_sel:[0,0] op_sel_hi:[1,1]"
#define MDCT_K_HL "op_sel:[0,1] op_sel_hi:[1,0]"
#define MDCT_X "op_sel:[0,1] op_sel_hi:[1,0]" // lo = a.lo (+) b.hi, hi = a.hi (+) b.lo
#define MDCT_NEG_B "neg_lo:[0,1] neg_hi:[0,1]"  // a - b in both halves

constexpr float kMagic23 = 12582912.0f, kQLo = kMagic23 - 32768.0f, kQHi = kMagic23 + 32767.0f;

// 8 pixels of one block row.  The reference takes any alignment (unaligned loads,
// simd_dct.cpp:2109); so does this: gfx950 global loads are alignment-free in hardware, the
// type below only stops the compiler from assuming 8-byte alignment.  Streamed once -> nt.
typedef unsigned int u32x2_unaligned __attribute__((ext_vector_type(2), aligned(1)));
__device__ __forceinline__ uint2 load8(const uint8_t *p)
{
  const u32x2_unaligned v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_unaligned *>(p));
  return make_uint2(v.x, v.y);
}

// byte N of a dword -> float in ONE instruction (v_cvt_f32_ubyteN).  Written as (pure,
// schedulable) inline asm, not as (float)((w >> 8N) & 0xFF): from the latter LLVM rewrites the
// first butterfly stage as integer SDWA adds followed by v_cvt_f32_i32 (exact, but ~1.6x the
// issue cycles on gfx950, where SDWA forms and converts are half rate).
template <int N>
__device__ __forceinline__ float ubyte_to_float(uint32_t w)
{
  float f;
  if constexpr (N == 0) asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(f) : "v"(w));
  else if constexpr (N == 1) asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(f) : "v"(w));
  else if constexpr (N == 2) asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(f) : "v"(w));
  else asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(f) : "v"(w));
  return f;
}

// The AAN butterflies on packed fp32 (fused round trip; profiles/r02_exp_i16_packed.log).  Same idea as the u8
// tiers above: rows "horizontally" on 4 register pairs with op_sel / neg modifiers, columns "vertically" on pairs of
// columns.  AAN's flow graph leaves 6 (forward) / 12 (inverse) operations per horizontal transform without a
// partner; they stay scalar.  Every packed or scalar operation is the individually rounded IEEE operation of
// aan_fwd8 / aan_inv8, so the results are bit-identical (and are tested as such against the CPU checker).
// The first ten floats of DctConsts are laid out as the pairs these functions consume.
struct AanPk
{
  f32x2 c707_382;   // (cos(pi/4), cos(3pi/8))
  f32x2 c541_1306;  // (cos(pi/8)-cos(3pi/8), cos(pi/8)+cos(3pi/8))
  f32x2 c1414_1847; // (sqrt 2, 2cos(pi/8))
  f32x2 c1082_2613;
  f32x2 magic;      // (1.5*2^23, 1.5*2^29)
};
static_assert(offsetof(DctConsts, c707) == 0 && offsetof(DctConsts, c382) == 4 && offsetof(DctConsts, c541) == 8 && offsetof(DctConsts, c1306) == 12 &&
                  offsetof(DctConsts, c1414) == 16 && offsetof(DctConsts, c1847) == 20 && offsetof(DctConsts, c1082) == 24 && offsetof(DctConsts, c2613) == 28 &&
                  offsetof(DctConsts, magic23) == 32 && offsetof(DctConsts, magic29) == 36,
              "AanPk views the head of DctConsts");


typedef const __attribute__((address_space(4))) char *kbytes_t;

// The two tables are 128 multiplier pairs = 256 SGPRs if the compiler is left to fetch them when it likes -- it fetches
// them all at the top and spills (252 v_readlane + 124 v_writelane per wave, 1451 vector instructions instead of ~1000).
// So the pairs of column pair j are read from the argument segment through a pointer the compiler cannot see through,
// right where they are used: two s_load_dwordx16 per j, 32 SGPRs live (mdct_api.hip lays the tables out j-major for this).
typedef const __attribute__((address_space(4))) f32x2 *karg_pairs_t;
__device__ __forceinline__ kbytes_t karg_bytes(size_t byte_off) { return (kbytes_t)__builtin_amdgcn_kernarg_segment_ptr() + byte_off; }
__device__ __forceinline__ karg_pairs_t karg_pairs(size_t byte_off) { return (karg_pairs_t)karg_bytes(byte_off); }

} // namespace mdct
