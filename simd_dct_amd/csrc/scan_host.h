// scan_host.h -- host checks and table building shared by the JPEG scan coders' entry points (jpeg_encode_scan.hip,
// jpeg_encode_opt.hip, jpeg_encode_batch.hip).  Include after host_error.h: every check leaves its message through that translation unit's fail().
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <mutex>

#include "mdct_jpegenc_opt.h"
#include "mdct_jpegenc_scan.h"
#include "own_tables.h"

namespace
{

// the three planes of an interleaved scan: *h, *v the luma sampling, the MCU grid from the chroma planes
[[maybe_unused]] int check_mcu_planes(const mdct_jpegenc_scan_plane *planes, int *h, int *v, size_t *mcus_x, size_t *mcus_y)
{
  for (int c = 0; c < 3; c++)
    if (!planes[c].px)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: null pointer", c);
  *h = planes[0].h;
  *v = planes[0].v;
  if (planes[1].h != 1 || planes[1].v != 1 || planes[2].h != 1 || planes[2].v != 1)
    return fail(MDCT_INVALID_PARAMETER, "chroma sampling factors %dx%d / %dx%d (1x1)", planes[1].h, planes[1].v, planes[2].h, planes[2].v);
  if (!((*h == 1 && *v == 1) || (*h == 2 && *v == 1) || (*h == 2 && *v == 2)))
    return fail(MDCT_INVALID_PARAMETER, "luma sampling factors %dx%d (1x1, 2x1 or 2x2)", *h, *v);
  *mcus_x = planes[1].width / 8;
  *mcus_y = planes[1].height / 8;
  for (int c = 0; c < 3; c++)
  {
    const mdct_jpegenc_scan_plane &p = planes[c];
    if (p.width == 0 || p.height == 0 || p.width > 65536 || p.height > 65536 || p.width != *mcus_x * 8 * (size_t)p.h || p.height != *mcus_y * 8 * (size_t)p.v)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: %zux%zu at sampling %dx%d is not on the MCU grid of %zux%zu MCUs the chroma planes state (width = mcus_x * 8 * h, "
                  "height = mcus_y * 8 * v, 8..65536)", c, p.width, p.height, p.h, p.v, *mcus_x, *mcus_y);
    if (p.pitch < p.width)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: pitch %zu < width %zu", c, p.pitch, p.width);
  }
  return MDCT_SUCCESS;
}

// one plane coded block row by block row
[[maybe_unused]] int check_block_plane(const uint8_t *px, size_t pitch, size_t width, size_t height, int c)
{
  if (!px)
    return fail(MDCT_INVALID_PARAMETER, "plane %d: null pointer", c);
  if (width == 0 || height == 0 || width % 8 || height % 8 || width > 65536 || height > 65536)
    return fail(MDCT_INVALID_PARAMETER, "plane %d: %zux%zu (multiples of 8, 8..65536)", c, width, height);
  if (pitch < width)
    return fail(MDCT_INVALID_PARAMETER, "plane %d: pitch %zu < width %zu", c, pitch, width);
  return MDCT_SUCCESS;
}

// a quantisation table -> the multiplier tables of the forward path, in the pair order of the column pass
[[maybe_unused]] int fill_lut(const float *lut, mdct::OwnTables &tb, const char *name)
{
  const int bad = mdct::own_tables_fill(lut, tb, /*pair_order=*/true);
  if (bad >= 0)
    return fail(MDCT_INVALID_PARAMETER, "%s table entry %d is %g; finite non-zero entries", name, bad, (double)lut[bad]);
  return MDCT_SUCCESS;
}

// the segment buffer: segments seg_stride apart, each with room for `need` = per_block * blocks + 8 bytes (rounded up to a dword by
// the caller where that is no multiple of 4); unit names what the blocks are counted over, why where per_block comes from
int check_seg_stride(size_t seg_stride, const void *out, size_t need, int per_block, size_t blocks, const char *unit, const char *why)
{
  if (seg_stride < need || seg_stride % 4 != 0 || ((uintptr_t)out & 3))
    return fail(MDCT_INVALID_PARAMETER, "seg_stride %zu: a multiple of 4 and >= %d * %zu blocks per %s + 8 = %zu (%s); out 4-byte aligned", seg_stride, per_block, blocks,
                unit, need, why);
  return MDCT_SUCCESS;
}

// T.81 Annex C: a table specification (the counts of codes of 1..16 bits, the values in code order) -> tab[value] = size << 16 | code
// for the values below cap.  Nothing is checked here: values without a code keep what tab held.
void annex_c_codes(const uint8_t *bits16, const uint8_t *vals, int nvals, int cap, uint32_t *tab)
{
  uint32_t code = 0;
  int k = 0;
  for (uint32_t len = 1; len <= 16; len++, code <<= 1)
    for (int i = 0; i < bits16[len - 1] && k < nvals; i++, k++, code++)
      if (vals[k] < cap)
        tab[vals[k]] = len << 16 | code;
}

// size << 16 | code of every symbol of the four Annex K tables (T.81 Annex C from mdct_huffman_spec), built once per process
struct HuffCodes
{
  uint32_t dc[2][12], ac[2][256];
  bool ok;
};

[[maybe_unused]] const HuffCodes &huff_codes()
{
  static HuffCodes t;
  static std::once_flag once;
  std::call_once(once, [] {
    memset(&t, 0, sizeof(t));
    t.ok = true;
    for (int which = 0; which < 4; which++)
    { // 0 DC luminance, 1 AC luminance, 2 DC chrominance, 3 AC chrominance
      uint8_t bits[16], vals[256];
      int nvals = 0;
      if (mdct_huffman_spec(which, bits, vals, &nvals) != MDCT_SUCCESS)
      {
        t.ok = false;
        return;
      }
      annex_c_codes(bits, vals, nvals, (which & 1) ? 256 : 12, (which & 1) ? t.ac[which >> 1] : t.dc[which >> 1]);
    }
  });
  return t;
}

// a specification -> size << 16 | code per symbol (T.81 Annex C); checked as mdct_jpegdec_tables_check checks one, and no symbol twice.
// complete: every baseline symbol of the class has a code.
[[maybe_unused]] int spec_codes(const mdct_jpegenc_opt_spec *sp, bool is_ac, const char *name, uint32_t *tab, bool *complete)
{
  const int cap = is_ac ? 256 : 12;
  memset(tab, 0, sizeof(uint32_t) * (size_t)cap);
  if (!sp || !sp->bits16 || !sp->vals)
    return fail(MDCT_INVALID_PARAMETER, "%s: null specification / counts / values", name);
  if (sp->nvals < 1 || sp->nvals > 256)
    return fail(MDCT_INVALID_PARAMETER, "%s: %d values (1..256)", name, sp->nvals);
  int total = 0;
  for (int l = 0; l < 16; l++)
    total += sp->bits16[l];
  if (total != sp->nvals)
    return fail(MDCT_INVALID_PARAMETER, "%s: the 16 counts add up to %d codes, %d values given", name, total, sp->nvals);
  uint32_t code = 0;
  bool seen[256] = {false};
  for (uint32_t l = 1, p = 0; l <= 16; l++)
  {
    const uint32_t n = sp->bits16[l - 1];
    for (uint32_t i = 0; i < n; i++, p++)
    {
      const int v = sp->vals[p];
      if (is_ac ? (v & 15) > 10 : v > 11)
        return fail(MDCT_INVALID_PARAMETER, "%s: value 0x%02x is not a baseline %s symbol", name, v, is_ac ? "AC" : "DC");
      if (seen[v])
        return fail(MDCT_INVALID_PARAMETER, "%s: value 0x%02x is named twice", name, v);
      seen[v] = true;
    }
    code += n;
    if (code >= (1u << l)) // no code may be all 1-bits, as libjpeg requires
      return fail(MDCT_INVALID_PARAMETER, "%s: codes over-subscribed at length %u", name, l);
    code <<= 1;
  }
  annex_c_codes(sp->bits16, sp->vals, sp->nvals, cap, tab);
  bool all = true;
  if (is_ac)
  {
    all = tab[0x00] && tab[0xF0];
    for (int r = 0; r < 16; r++)
      for (int s = 1; s <= 10; s++)
        all = all && tab[r << 4 | s];
  }
  else
    for (int s = 0; s < 12; s++)
      all = all && tab[s];
  *complete = *complete && all;
  return MDCT_SUCCESS;
}

} // namespace
