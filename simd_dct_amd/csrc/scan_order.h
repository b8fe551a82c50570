// scan_order.h -- how the chunked JPEG scan coders (scan_chunks.h: k_scan_rows, k_opt) lay a chunk of an MCU row out over a
// workgroup, and the permutation between that layout and the scan order of ITU-T T.81 A.2.3.  Pure index arithmetic, nothing of the
// HIP runtime: tests/scan_order_driver.cpp builds it with plain g++ (sanitizers on) and holds every thread of every layout against a
// statement of A.2.3 of its own.
//
// <H, V> is the luma sampling of an interleaved scan (chroma is 1x1) -- 4:2:0 <2, 2>, 4:2:2 <2, 1>, 4:4:4 <1, 1> -- or <0, 0>: ONE
// plane, an "MCU" is one block.  In the transform phase lane = block and waves are component-uniform (slot = wave * 64 + lane):
//   4:2:0  wave 0 / 1: the upper / lower luma block row, blocks 2 m0 .. 2 m0 + 63; wave 2: Cb m0 .. m0 + 31 | Cr the same
//   4:2:2  wave 0: luma; wave 1: Cb | Cr                                                      (kMcus = 32)
//   4:4:4  wave 0 Y, wave 1 Cb, wave 2 Cr, blocks m0 .. m0 + 63                               (kMcus = 64)
//   plane  waves 0..3: blocks m0 .. m0 + 255                                                  (kMcus = 256)
#ifndef MDCT_SCAN_ORDER_H
#define MDCT_SCAN_ORDER_H

#include <stdint.h>

#include "batch_plan.h" // MDCT_HD

namespace mdct
{
namespace scan_order
{

template <int H, int V> constexpr int kBlocksPerMcu = H == 0 ? 1 : H * V + 2;
template <int H, int V> constexpr int kWaves = H == 0 ? 4 : H == 2 ? V + 1 : 3;              // one plane 4, 4:2:0 3, 4:2:2 2, 4:4:4 3
template <int H, int V> constexpr uint32_t kMcus = H == 0 ? 256u : H == 2 ? 32u : 64u;       // MCUs per chunk: 64 * kWaves blocks

// where the s-th block of a chunk in scan order was transformed (slot = wave * 64 + lane), where its predecessor of the same component
// was (pred; carry: it is the component's last block of the previous chunk), and whether it is a chroma block
struct SeqBlock
{
  uint32_t mcu, slot, pred;
  bool carry, chroma;
};

template <int H, int V>
MDCT_HD SeqBlock seq_block(uint32_t s)
{
  constexpr uint32_t B = kBlocksPerMcu<H, V>, M = kMcus<H, V>;
  const uint32_t i = s / B, k = s - i * B;
  SeqBlock b;
  b.mcu = i;
  if constexpr (H == 0)
  { // one plane: lane order
    b.chroma = false;
    b.slot = s;
    b.carry = s == 0;
    b.pred = b.carry ? M - 1 : s - 1;
  }
  else if constexpr (H == 1)
  { // Y Cb Cr: wave k, lane i
    b.chroma = k > 0;
    b.slot = k * 64 + i;
    b.carry = i == 0;
    b.pred = b.carry ? k * 64 + 63 : b.slot - 1;
  }
  else
  {
    constexpr uint32_t NY = H * V, C0 = 64 * V; // luma blocks per MCU, the chroma wave's first slot
    b.chroma = k >= NY;
    if (k >= NY)
    { // Cb: lanes 0..31 of the chroma wave, Cr: lanes 32..63
      const uint32_t first = C0 + (k - NY) * M;
      b.slot = first + i;
      b.carry = i == 0;
      b.pred = b.carry ? first + M - 1 : b.slot - 1;
    }
    else if constexpr (V == 1)
    { // Y0 Y1: lanes 2i, 2i + 1 of wave 0
      b.slot = 2 * i + k;
      b.carry = b.slot == 0;
      b.pred = b.carry ? 63 : b.slot - 1;
    }
    else
    { // Y00 Y01 Y10 Y11: wave k >> 1 (the luma block row), lane 2i + (k & 1)
      b.slot = (k >> 1) * 64 + 2 * i + (k & 1);
      b.carry = s == 0;
      // Y00 follows the previous MCU's Y11, Y01 Y00, Y10 Y01, Y11 Y10
      b.pred = k == 0 ? (b.carry ? 127 : 64 + 2 * i - 1) : k == 1 ? 2 * i : k == 2 ? 2 * i + 1 : 64 + 2 * i;
    }
  }
  return b;
}

} // namespace scan_order
} // namespace mdct

#endif
