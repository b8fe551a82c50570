// huff_tables.h -- the JPEG decoders' Huffman tables as the kernels read them (jpegdec_common.h: huff()), built on the host from DHT
// specifications (mdct_jpegdec_tables_check / _create).  Nothing of the HIP runtime: tests/jpegdec_host_driver.cpp builds it with plain
// g++ (sanitizers on), decodes every code of a table both ways and hands it the specifications it has to refuse.
#ifndef MDCT_HUFF_TABLES_H
#define MDCT_HUFF_TABLES_H

#include <stdint.h>
#include <string.h>

#include "host_error.h"
#include "mdct.h"

namespace mdct
{
namespace jpegdec
{

constexpr int kFastBits = 9; // codes up to 9 bits resolve in one LDS lookup

// T.81 C.2 / F.2.2.3, built on the host: fast[peek9] = (length << 8) | value for codes of <= 9 bits (0: longer code or none);
// a 16-bit left-justified code c has length l if c < limit[l] (first such l), and its value is vals[(c >> (16 - l)) + delta[l]].
struct DevTables
{
  uint16_t fast[4][1 << kFastBits];
  int32_t limit[4][18];
  int32_t delta[4][18];
  uint8_t vals[4][256];
};
static_assert(sizeof(DevTables) % 4 == 0, "LDS copy in words");

// the four slots' specifications (bits16[t] null: slot t empty) checked and, with `out`, built; a refusal leaves `out` partly written
static inline int build_tables(const uint8_t *const bits16[4], const uint8_t *const vals[4], const int nvals[4], DevTables *out, bool present[4])
{
  if (!bits16 || !vals || !nvals)
    return fail(MDCT_INVALID_PARAMETER, "null table arrays");
  if (out)
    memset(out, 0, sizeof(*out));
  for (int t = 0; t < 4; t++)
  {
    present[t] = bits16[t] != nullptr;
    if (!present[t])
      continue;
    if (!vals[t] && nvals[t] > 0)
      return fail(MDCT_INVALID_PARAMETER, "slot %d: null values", t);
    if (nvals[t] < 0 || nvals[t] > 256)
      return fail(MDCT_INVALID_PARAMETER, "slot %d: %d values (at most 256)", t, nvals[t]);
    int total = 0;
    for (int l = 0; l < 16; l++)
      total += bits16[t][l];
    if (total != nvals[t])
      return fail(MDCT_INVALID_PARAMETER, "slot %d: the 16 counts add up to %d codes, %d values given", t, total, nvals[t]);
    for (int i = 0; i < total; i++)
    {
      const int v = vals[t][i];
      if (t < 2 ? v > 11 : (v & 15) > 10)
        return fail(MDCT_INVALID_PARAMETER, "slot %d: value 0x%02x is not a baseline %s symbol", t, v, t < 2 ? "DC" : "AC");
    }
    // canonical codes (C.2); no code may be all 1-bits, as libjpeg requires
    int code = 0, p = 0;
    for (int l = 1; l <= 16; l++)
    {
      const int n = bits16[t][l - 1];
      // (before anything is written for this length: its codes index fast[])
      if (code + n >= (1 << l))
        return fail(MDCT_INVALID_PARAMETER, "slot %d: codes over-subscribed at length %d", t, l);
      if (out)
      {
        out->limit[t][l] = n ? (code + n) << (16 - l) : 0;
        out->delta[t][l] = p - code;
        if (l <= kFastBits)
          for (int i = 0; i < n; i++)
            for (int f = (code + i) << (kFastBits - l); f < (code + i + 1) << (kFastBits - l); f++)
              out->fast[t][f] = (uint16_t)((l << 8) | vals[t][p + i]);
      }
      code = (code + n) << 1;
      p += n;
    }
    if (out)
    {
      out->limit[t][17] = 0x7FFFFFFF;
      if (total)
        memcpy(out->vals[t], vals[t], (size_t)total);
    }
  }
  return MDCT_SUCCESS;
}

} // namespace jpegdec
} // namespace mdct

#endif
