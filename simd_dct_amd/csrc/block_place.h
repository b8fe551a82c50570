// block_place.h -- where the JPEG decoders (jpegdec_common.h) put the blocks of a scan: the layout of an MCU over up to three
// coefficient planes, the place of a block (ITU-T T.81 A.2.3) and the loop that zeroes a range of blocks.  Nothing of the HIP runtime:
// tests/jpegdec_host_driver.cpp builds it with plain g++ (sanitizers on) and holds five layouts against a statement of A.2.3 of its own.
#ifndef MDCT_BLOCK_PLACE_H
#define MDCT_BLOCK_PLACE_H

#include <stdint.h>
#include <string.h>

#include "batch_plan.h" // MDCT_HD
#include "mdct_jpegdec.h"

namespace mdct
{
namespace jpegdec
{

// One scan's block layout (DecArgs embeds it): block b of an MCU is block (bh[b], bv[b]) of component bcomp[b]'s ch x cv blocks of the
// MCU; rows of plane c lie pitch[c] elements apart
struct BlockPlace
{
  int16_t *plane[3];
  uint64_t pitch[3];
  uint32_t upm; // blocks per MCU
  uint8_t bcomp[MDCT_JPEGDEC_MAX_BLOCKS_PER_MCU], bh[MDCT_JPEGDEC_MAX_BLOCKS_PER_MCU], bv[MDCT_JPEGDEC_MAX_BLOCKS_PER_MCU];
  uint32_t ch[3], cv[3]; // h, v per component
  uint32_t mcus_x;
};

// first element of row `row` of block b (component c = bcomp[b], which the decoder keeps in LDS) of the MCU in column mx, row my
MDCT_HD int16_t *block_at(const BlockPlace &g, uint32_t mx, uint32_t my, uint32_t b, uint32_t c, uint32_t row)
{
  return g.plane[c] + ((size_t)(my * g.cv[c] + g.bv[b]) * 8 + row) * g.pitch[c] + (size_t)(mx * g.ch[c] + g.bh[b]) * 8;
}

// Zero units (blocks in decoding order) [z0, z0 + nz) of the interval that starts at MCU mcu0, as 8 row stores of 16 bytes per unit (rows
// are 16-byte aligned).  Store wi of the nz * 8 is row wi / nz of unit z0 + wi % nz, and the caller does first, first + stride, ...:
// consecutive lanes on consecutive numbers store to consecutive blocks of one pixel row.  I counts the stores: nz * 8 + stride must fit.
template <class I>
MDCT_HD void zero_units(const BlockPlace &g, uint32_t mcu0, uint32_t z0, uint32_t nz, I first, I stride)
{
  for (I wi = first; wi < (I)nz * 8; wi += stride)
  {
    const uint32_t row = (uint32_t)(wi / nz), unit = z0 + (uint32_t)(wi - (I)row * nz);
    const uint32_t mcu = mcu0 + unit / g.upm, b = unit % g.upm, my = mcu / g.mcus_x; // unit -> block b of MCU mcu
    memset(__builtin_assume_aligned(block_at(g, mcu - my * g.mcus_x, my, b, g.bcomp[b], row), 16), 0, 16);
  }
}

} // namespace jpegdec
} // namespace mdct

#endif
