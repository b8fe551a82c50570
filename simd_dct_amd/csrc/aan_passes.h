// aan_passes.h -- the engine-own AAN passes on packed fp32 as asm blocks (aan_fwd_v, aan_inv_v, aan_fwd_h, aan_inv_h) and the back half
// of the fused pixels -> Huffman rows kernels built on them: the column passes with the quantiser (fwd_v_quant_levels) and the zig-zag
// compaction (compact_levels16).  mdct_kernels.hip (libmdct_hip.so) includes it, and so do the JPEG scan coders -- jpeg_encode_scan.hip,
// jpeg_encode_opt.hip, jpeg_coef.hip, each its own library -- for the chunk skeleton they share (scan_chunks.h): one text, the same
// coefficients by construction.  tests/test_asm_blocks.py proves the four blocks from this file, operation for operation, against the
// scalar definition (aan_fwd8 / aan_inv8, mdct_kernels.hip).  Device code only.
#pragma once
#include "aan_fwd.h"
#include "scan_records.h"

#pragma clang fp contract(off)

namespace mdct
{

// ---------------------------------------------------------------------------------------
// The four passes are ASM BLOCKS, not one asm statement per operation (MDCT_PKA / MDCT_PKM / MDCT_PKF, aan_fwd.h), which is how they
// were first written.  One asm statement per operation cost wait states the hardware does not need: for an asm statement that reads a VGPR
// written by the asm statement right before it the compiler inserts an s_nop (it cannot see inside and assumes the gfx940 dst_sel
// forwarding hazard, which a v_pk_*_f32 does not have) -- 97 of them per wave in k_u8_batch, 60-70 in the int16 round trip, each an issue
// slot.  The column passes are pure packed sequences: one block of 30 instructions each, registers allocated by hand, results left in a
// PERMUTATION of the input registers (renaming is free for the caller).  The row passes keep their 6 / 12 unpaired scalar operations as
// compiler-visible code (an inline-asm operand cannot name half of a register pair) between two blocks of packed operations.
// Same operations, same operands, same order of operands in every subtraction as the scalar definition (aan_fwd8 / aan_inv8).
// ---------------------------------------------------------------------------------------
#define MDCT_XSEL " op_sel:[0,1] op_sel_hi:[1,0]" // lo = a.lo (+) b.hi, hi = a.hi (+) b.lo (MDCT_X inside a block)
#define MDCT_SUB " neg_lo:[0,1] neg_hi:[0,1]\n\t"
#define MDCT_KLO " op_sel:[0,0] op_sel_hi:[1,0]\n\t" // times the constant pair's low half, both halves
#define MDCT_KHI " op_sel:[0,1] op_sel_hi:[1,1]\n\t" // times its high half
// v_pk_fma_f32 d, a, k, c: a * (the constant pair's low / high half, both halves) + c; _NA negates a (-a k + c), _NC negates c (a k - c)
#define MDCT_FKLO " op_sel:[0,0,0] op_sel_hi:[1,0,1]\n\t"
#define MDCT_FKHI " op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
#define MDCT_FKLO_NA " op_sel:[0,0,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"
#define MDCT_FKHI_NA " op_sel:[0,1,0] op_sel_hi:[1,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"
#define MDCT_FKLO_NC " op_sel:[0,0,0] op_sel_hi:[1,0,1] neg_lo:[0,0,1] neg_hi:[0,0,1]\n\t"

__device__ __forceinline__ void aan_fwd_v(const AanPk &K, f32x2 (&p)[8])
{
  f32x2 r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3], r4 = p[4], r5 = p[5], r6 = p[6], r7 = p[7], T;
  asm("v_pk_add_f32 %8, %0, %7\n\t"            /* T  = t0 = p0 + p7 */
      "v_pk_add_f32 %7, %0, %7" MDCT_SUB       /* r7 = t7 = p0 - p7 */
      "v_pk_add_f32 %0, %1, %6\n\t"            /* r0 = t1 */
      "v_pk_add_f32 %6, %1, %6" MDCT_SUB       /* r6 = t6 */
      "v_pk_add_f32 %1, %2, %5\n\t"            /* r1 = t2 */
      "v_pk_add_f32 %5, %2, %5" MDCT_SUB       /* r5 = t5 */
      "v_pk_add_f32 %2, %3, %4\n\t"            /* r2 = t3 */
      "v_pk_add_f32 %4, %3, %4" MDCT_SUB       /* r4 = t4 */
      "v_pk_add_f32 %3, %8, %2\n\t"            /* r3 = e10 = t0 + t3 */
      "v_pk_add_f32 %2, %8, %2" MDCT_SUB       /* r2 = e13 = t0 - t3 */
      "v_pk_add_f32 %8, %0, %1\n\t"            /* T  = e11 = t1 + t2 */
      "v_pk_add_f32 %1, %0, %1" MDCT_SUB       /* r1 = e12 = t1 - t2 */
      "v_pk_add_f32 %0, %3, %8\n\t"            /* r0 = out0 = e10 + e11 */
      "v_pk_add_f32 %8, %3, %8" MDCT_SUB       /* T  = out4 = e10 - e11 */
      "v_pk_add_f32 %3, %1, %2\n\t"            /* r3 = s1 = e12 + e13 */
      "v_pk_add_f32 %1, %4, %5\n\t"            /* r1 = o10 = t4 + t5            (e12 is dead) */
      "v_pk_add_f32 %4, %5, %6\n\t"            /* r4 = o11 = t5 + t6 */
      "v_pk_add_f32 %5, %6, %7\n\t"            /* r5 = o12 = t6 + t7 */
      "v_pk_fma_f32 %6, %3, %9, %2" MDCT_FKLO_NA /* r6 = out6 = -s1 c707 + e13 */
      "v_pk_fma_f32 %2, %3, %9, %2" MDCT_FKLO    /* r2 = out2 = s1 c707 + e13 */
      "v_pk_add_f32 %3, %1, %5" MDCT_SUB       /* r3 = o10 - o12 */
      "v_pk_mul_f32 %3, %3, %9" MDCT_KHI       /* r3 = z5 = (o10 - o12) c382 */
      "v_pk_fma_f32 %1, %1, %10, %3" MDCT_FKLO   /* r1 = z2 = o10 c541 + z5 */
      "v_pk_fma_f32 %5, %5, %10, %3" MDCT_FKHI   /* r5 = z4 = o12 c1306 + z5 */
      "v_pk_fma_f32 %3, %4, %9, %7" MDCT_FKLO    /* r3 = z11 = o11 c707 + t7 */
      "v_pk_fma_f32 %7, %4, %9, %7" MDCT_FKLO_NA /* r7 = z13 = -o11 c707 + t7 */
      "v_pk_add_f32 %4, %7, %1\n\t"            /* r4 = out5 = z13 + z2 */
      "v_pk_add_f32 %7, %7, %1" MDCT_SUB       /* r7 = out3 = z13 - z2 */
      "v_pk_add_f32 %1, %3, %5\n\t"            /* r1 = out1 = z11 + z4 */
      "v_pk_add_f32 %3, %3, %5 neg_lo:[0,1] neg_hi:[0,1]" /* r3 = out7 = z11 - z4 */
      : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6), "+v"(r7), "=&v"(T)
      : "s"(K.c707_382), "s"(K.c541_1306));
  p[0] = r0; p[1] = r1; p[2] = r2; p[3] = r7; p[4] = T; p[5] = r4; p[6] = r6; p[7] = r3;
}

__device__ __forceinline__ void aan_inv_v(const AanPk &K, f32x2 (&p)[8])
{
  f32x2 r0 = p[0], r1 = p[1], r2 = p[2], r3 = p[3], r4 = p[4], r5 = p[5], r6 = p[6], r7 = p[7], T;
  asm("v_pk_add_f32 %8, %0, %4\n\t"            /* T  = e10 = p0 + p4 */
      "v_pk_add_f32 %4, %0, %4" MDCT_SUB       /* r4 = e11 = p0 - p4 */
      "v_pk_add_f32 %0, %2, %6\n\t"            /* r0 = e13 = p2 + p6 */
      "v_pk_add_f32 %6, %2, %6" MDCT_SUB       /* r6 = p2 - p6 */
      "v_pk_add_f32 %2, %5, %3\n\t"            /* r2 = z13 = p5 + p3 */
      "v_pk_add_f32 %3, %5, %3" MDCT_SUB       /* r3 = z10 = p5 - p3 */
      "v_pk_add_f32 %5, %1, %7\n\t"            /* r5 = z11 = p1 + p7 */
      "v_pk_add_f32 %7, %1, %7" MDCT_SUB       /* r7 = z12 = p1 - p7 */
      "v_pk_fma_f32 %6, %6, %9, %0" MDCT_FKLO_NC /* r6 = e12 = (p2 - p6) c1414 - e13 */
      "v_pk_add_f32 %1, %5, %2\n\t"            /* r1 = t7 = z11 + z13 */
      "v_pk_add_f32 %5, %5, %2" MDCT_SUB       /* r5 = z11 - z13 */
      "v_pk_add_f32 %2, %3, %7\n\t"            /* r2 = z10 + z12 */
      "v_pk_mul_f32 %2, %2, %9" MDCT_KHI       /* r2 = z5 = (z10 + z12) c1847 */
      "v_pk_fma_f32 %7, %7, %10, %2" MDCT_FKLO_NC /* r7 = o10 = z12 c1082 - z5 */
      "v_pk_fma_f32 %3, %3, %10, %2" MDCT_FKHI_NA /* r3 = o12 = -z10 c2613 + z5 */
      "v_pk_add_f32 %2, %8, %0\n\t"            /* r2 = t0 = e10 + e13 */
      "v_pk_add_f32 %0, %8, %0" MDCT_SUB       /* r0 = t3 = e10 - e13 */
      "v_pk_add_f32 %3, %3, %1" MDCT_SUB       /* r3 = t6 = o12 - t7 */
      "v_pk_add_f32 %8, %4, %6\n\t"            /* T  = t1 = e11 + e12 */
      "v_pk_add_f32 %6, %4, %6" MDCT_SUB       /* r6 = t2 = e11 - e12 */
      "v_pk_fma_f32 %5, %5, %9, %3" MDCT_FKLO_NC /* r5 = t5 = (z11 - z13) c1414 - t6 */
      "v_pk_add_f32 %4, %2, %1\n\t"            /* r4 = out0 = t0 + t7 */
      "v_pk_add_f32 %2, %2, %1" MDCT_SUB       /* r2 = out7 = t0 - t7 */
      "v_pk_add_f32 %7, %7, %5\n\t"            /* r7 = t4 = o10 + t5 */
      "v_pk_add_f32 %1, %8, %3\n\t"            /* r1 = out1 = t1 + t6 */
      "v_pk_add_f32 %8, %8, %3" MDCT_SUB       /* T  = out6 = t1 - t6 */
      "v_pk_add_f32 %3, %6, %5\n\t"            /* r3 = out2 = t2 + t5 */
      "v_pk_add_f32 %6, %6, %5" MDCT_SUB       /* r6 = out5 = t2 - t5 */
      "v_pk_add_f32 %5, %0, %7\n\t"            /* r5 = out4 = t3 + t4 */
      "v_pk_add_f32 %0, %0, %7 neg_lo:[0,1] neg_hi:[0,1]" /* r0 = out3 = t3 - t4 */
      : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3), "+v"(r4), "+v"(r5), "+v"(r6), "+v"(r7), "=&v"(T)
      : "s"(K.c1414_1847), "s"(K.c1082_2613));
  p[0] = r4; p[1] = r1; p[2] = r3; p[3] = r0; p[4] = r5; p[5] = r6; p[6] = T; p[7] = r2;
}

// forward, one line in natural pairs (p0,p1)(p2,p3)(p4,p5)(p6,p7) -> (y0,y4) (y2,y6) (y5,y3) (y1,y7)
__device__ __forceinline__ void aan_fwd_h(const AanPk &K, f32x2 a01, f32x2 a23, f32x2 a45, f32x2 a67, f32x2 &o04, f32x2 &o26, f32x2 &o53, f32x2 &o17)
{
  f32x2 T0, T1;
  asm("v_pk_add_f32 %4, %0, %3" MDCT_XSEL "\n\t"                               /* T0 = (t0, t1) = (p0+p7, p1+p6) */
      "v_pk_add_f32 %5, %1, %2" MDCT_XSEL "\n\t"                               /* T1 = (t2, t3) = (p2+p5, p3+p4) */
      "v_pk_add_f32 %0, %0, %3" MDCT_XSEL " neg_lo:[0,1] neg_hi:[0,1]\n\t"     /* A  = (t7, t6) = (p0-p7, p1-p6) */
      "v_pk_add_f32 %1, %1, %2" MDCT_XSEL " neg_lo:[0,1] neg_hi:[0,1]\n\t"     /* B  = (t5, t4) = (p2-p5, p3-p4) */
      "v_pk_add_f32 %2, %4, %5" MDCT_XSEL "\n\t"                               /* C  = (e10, e11) = (t0+t3, t1+t2) */
      "v_pk_add_f32 %3, %4, %5" MDCT_XSEL " neg_lo:[0,1] neg_hi:[0,1]\n\t"     /* D  = (e13, e12) = (t0-t3, t1-t2) */
      "v_pk_add_f32 %4, %2, %2 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]"      /* T0 = (e10+e11, e10-e11) */
      : "+v"(a01), "+v"(a23), "+v"(a45), "+v"(a67), "=&v"(T0), "=&v"(T1));
  const f32x2 t76 = a01, t54 = a23, e32 = a67;
  o04 = T0;
  f32x2 w, o, z5;
  w.x = e32.y + e32.x;                               // s1 = e12 + e13
  w.y = t54.x + t76.y;                               // o11 = t5 + t6
  o.x = t54.y + t54.x;                               // o10 = t4 + t5
  o.y = t76.y + t76.x;                               // o12 = t6 + t7
  z5.x = (o.x - o.y) * K.c707_382.y;                 // z5 = (o10 - o12) * c382
  z5.y = z5.x;
  f32x2 T;
  asm("v_pk_fma_f32 %1, %1, %9, %7 op_sel:[0,0,0] op_sel_hi:[1,1,0]\n\t"                  /* o  = (z2, z4) = (o10 c541 + z5, o12 c1306 + z5) */
      "v_pk_fma_f32 %2, %0, %8, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0] neg_hi:[1,0,0]\n\t"   /* T  = (z11, z13) = (o11 c707 + t7, -o11 c707 + t7) */
      "v_pk_fma_f32 %3, %0, %8, %6 op_sel:[0,0,0] op_sel_hi:[0,0,0] neg_hi:[1,0,0]\n\t"   /* o26 = (s1 c707 + e13, -s1 c707 + e13) */
      "v_pk_add_f32 %4, %2, %1 op_sel:[1,0] op_sel_hi:[1,0] neg_hi:[0,1]\n\t"             /* o53 = (z13+z2, z13-z2) */
      "v_pk_add_f32 %2, %2, %1 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]"                 /* T -> o17 = (z11+z4, z11-z4) */
      : "+v"(w), "+v"(o), "=&v"(T), "=&v"(o26), "=&v"(o53)
      : "v"(t76), "v"(e32), "v"(z5), "s"(K.c707_382), "s"(K.c541_1306));
  o17 = T;
}

// inverse, one line given as (c0,c4) (c2,c6) (c5,c3) (c1,c7) -> (x0,x7) (x1,x6) (x2,x5) (x4,x3)
__device__ __forceinline__ void aan_inv_h(const AanPk &K, f32x2 i04, f32x2 i26, f32x2 i53, f32x2 i17, f32x2 &o07, f32x2 &o16, f32x2 &o25, f32x2 &o43)
{
  f32x2 td;
  asm("v_pk_add_f32 %0, %0, %0 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]\n\t"  /* e  = (e10, e11) = (c0+c4, c0-c4) */
      "v_pk_add_f32 %1, %1, %1 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]\n\t"  /* f  = (e13, c2-c6) */
      "v_pk_add_f32 %2, %2, %2 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]\n\t"  /* z3 = (z13, z10) = (c5+c3, c5-c3) */
      "v_pk_add_f32 %3, %3, %3 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[0,1]\n\t"  /* z1 = (z11, z12) = (c1+c7, c1-c7) */
      "v_pk_add_f32 %4, %3, %2 op_sel:[0,0] op_sel_hi:[0,0] neg_hi:[0,1]"      /* td = (t7, z11-z13) */
      : "+v"(i04), "+v"(i26), "+v"(i53), "+v"(i17), "=&v"(td));
  f32x2 f = i26, u;
  f.y = __builtin_fmaf(f.y, K.c1414_1847.x, -f.x);       // e12 = (c2-c6)*sqrt2 - e13, fused
  const float z5 = (i53.y + i17.y) * K.c1414_1847.y;     // (z10 + z12) * c1847
  const float o10 = __builtin_fmaf(K.c1082_2613.x, i17.y, -z5);
  const float o12 = __builtin_fmaf(-K.c1082_2613.y, i53.y, z5);
  u.x = o12 - td.x;                                      // t6
  u.y = __builtin_fmaf(td.y, K.c1414_1847.x, -u.x);      // t5 = (z11-z13)*sqrt2 - t6, fused
  td.y = o10 + u.y;                                      // t4 (z11-z13 is dead: its half of td carries t4 into the block below)
  f32x2 t03, t12;
  asm("v_pk_add_f32 %4, %6, %7 op_sel:[0,0] op_sel_hi:[0,0] neg_hi:[0,1]\n\t"  /* t03 = (t0, t3) = (e10+e13, e10-e13) */
      "v_pk_add_f32 %5, %6, %7 op_sel:[1,1] op_sel_hi:[1,1] neg_hi:[0,1]\n\t"  /* t12 = (t1, t2) = (e11+e12, e11-e12) */
      "v_pk_add_f32 %0, %4, %8 op_sel:[0,0] op_sel_hi:[0,0] neg_hi:[0,1]\n\t"  /* o07 = (t0+t7, t0-t7) */
      "v_pk_add_f32 %3, %4, %8 op_sel:[1,1] op_sel_hi:[1,1] neg_hi:[0,1]\n\t"  /* o43 = (t3+t4, t3-t4) */
      "v_pk_add_f32 %1, %5, %9 op_sel:[0,0] op_sel_hi:[0,0] neg_hi:[0,1]\n\t"  /* o16 = (t1+t6, t1-t6) */
      "v_pk_add_f32 %2, %5, %9 op_sel:[1,1] op_sel_hi:[1,1] neg_hi:[0,1]"      /* o25 = (t2+t5, t2-t5) */
      : "=&v"(o07), "=&v"(o16), "=&v"(o25), "=&v"(o43), "=&v"(t03), "=&v"(t12)
      : "v"(i04), "v"(f), "v"(td), "v"(u));
}

// ---------------------------------------------------------------------------------------
// The back half of the fused pixels -> Huffman rows kernels, after the row passes left the block in P (aan_fwd_h).
// ---------------------------------------------------------------------------------------
// Column passes and quantiser: quantised levels as the low 16 bits of val[] (natural order v*8+u): the DC like the int16 plane would
// hold it (sat_i16), the AC coefficients saturated to the +-1023 of baseline categories 1..10 -- exactly what the staged coder does to
// an int16 record at token time.  qf: the 32 multiplier pairs in the pair order of the column pass (make_own_tables, pair_order), in
// the kernel's argument segment; dc_shift: 64 * 128 with the level shift (exactly "raw DC minus 64 * 128"), else 0.
// CLAMP = false: the caller knows that no level can leave those ranges, and the 64 saturations per block are left out.
template <bool CLAMP>
__device__ __forceinline__ void fwd_v_quant_levels(const AanPk &K, f32x2 (&P)[4][8], karg_pairs_t qf, float dc_shift, uint32_t (&val)[64])
{
  constexpr int kA[4] = {0, 2, 5, 1}, kB[4] = {4, 6, 3, 7};
  const f32x2 magic_v = K.magic;
#pragma unroll
  for (int j = 0; j < 4; j++)
  {
    aan_fwd_v(K, P[j]);
    if (j == 0)
      P[0][0].x = P[0][0].x - dc_shift;
    // the 8 multiplier pairs of column pair j, fetched here (all 64 multipliers held in SGPRs from the top of the kernel spilled)
    karg_pairs_t tq = qf + j * 8;
    asm volatile("" : "+s"(tq));
#pragma unroll
    for (int v = 0; v < 8; v++)
    {
      f32x2 c;
      MDCT_PKF(c, P[j][v], tq[v], magic_v, "op_sel:[0,0,0] op_sel_hi:[1,1,0]"); // quant_i16_bits; the clamps (baseline JPEG: AC to +-1023) on the biased value
      const bool is_dc = j == 0 && v == 0;
      if constexpr (CLAMP)
        c = f32x2{__builtin_amdgcn_fmed3f(c.x, is_dc ? kQLo : kMagic23 - 1023.0f, is_dc ? kQHi : kMagic23 + 1023.0f), __builtin_amdgcn_fmed3f(c.y, kMagic23 - 1023.0f, kMagic23 + 1023.0f)};
      val[v * 8 + kA[j]] = __float_as_uint(c.x);
      val[v * 8 + kB[j]] = __float_as_uint(c.y);
    }
  }
}

// Zig-zag order; AC entries run << 12 | level compacted to the front of the lane's LDS row rec (kRec16Row halfwords), a ZRL entry for
// every 16 zeros in a row.  EVERY coefficient writes run << 12 | level at the current position and only those that need an entry
// advance it: a zero's write is overwritten by the next entry -- unless it is the 16th zero in a row, and then what it
// wrote, 15 << 12 | 0, IS the ZRL entry.  (7 vector instructions per coefficient; selecting value and address per
// coefficient and tracking the last non-zero took 11.)  Returns the number of entries; ZRL entries after the last coefficient are
// dropped (at most three: 62 zeros).  my_dc: the DC level; need_eob: position 63 is not coded.
__device__ __forceinline__ uint32_t compact_levels16(const uint32_t (&val)[64], uint16_t *rec, int &my_dc, bool &need_eob)
{
  uint32_t pos = 0, r12 = 0;
#pragma unroll
  for (int k = 1; k < 64; k++)
  {
    const uint32_t v = val[kZigZag[k]];
    const bool nz = (v & 0xFFFFu) != 0;
    const bool wr = nz || r12 == 0xF000u;
    rec[pos] = (uint16_t)((v & 0xFFFu) | r12);
    pos += wr ? 1u : 0u;
    r12 = wr ? 0u : r12 + 0x1000u;
  }
  uint32_t n = pos;
#pragma unroll
  for (int t = 0; t < 3; t++)
    n -= (n > 0 && rec[n - 1] == 0xF000u) ? 1u : 0u;
  my_dc = (int)(int16_t)(val[0] & 0xFFFFu);
  need_eob = (val[kZigZag[63]] & 0xFFFFu) == 0;
  return n;
}

} // namespace mdct
