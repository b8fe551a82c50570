// coef_host.h -- host checks shared by the entry points that take coefficient planes (jpeg_coef.hip, jpeg_progressive.hip).
// Include after host_error.h: every check leaves its message through that translation unit's fail().
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "mdct_jpegcoef.h"

namespace
{

// one coefficient plane: pointer, alignment, pitch, grid
[[maybe_unused]] int check_coef_plane(const mdct_jpegcoef_plane &p, const char *what, int c)
{
  if (!p.coef)
    return fail(MDCT_INVALID_PARAMETER, "%s %d: null pointer", what, c);
  if ((uintptr_t)p.coef & 15)
    return fail(MDCT_INVALID_PARAMETER, "%s %d: coef is not 16-byte aligned", what, c);
  if (p.blocks_x == 0 || p.blocks_y == 0 || p.blocks_x > 65535 || p.blocks_y > 65535)
    return fail(MDCT_INVALID_PARAMETER, "%s %d: %u x %u blocks (1..65535 each way)", what, c, p.blocks_x, p.blocks_y);
  if (p.pitch % 8 != 0 || p.pitch < (size_t)p.blocks_x * 8)
    return fail(MDCT_INVALID_PARAMETER, "%s %d: pitch %zu elements (a multiple of 8, >= blocks_x * 8 = %zu)", what, c, p.pitch, (size_t)p.blocks_x * 8);
  return MDCT_SUCCESS;
}

// the three planes of an interleaved scan: *h, *v the luma sampling, the MCU grid from the chroma planes
[[maybe_unused]] int check_coef_mcu_planes(const mdct_jpegcoef_plane *planes, int *h, int *v, uint32_t *mcus_x, uint32_t *mcus_y)
{
  for (int c = 0; c < 3; c++)
    if (const int rc = check_coef_plane(planes[c], "plane", c))
      return rc;
  *h = planes[0].h;
  *v = planes[0].v;
  if (planes[1].h != 1 || planes[1].v != 1 || planes[2].h != 1 || planes[2].v != 1)
    return fail(MDCT_INVALID_PARAMETER, "chroma sampling factors %dx%d / %dx%d (1x1)", planes[1].h, planes[1].v, planes[2].h, planes[2].v);
  if (!((*h == 1 && *v == 1) || (*h == 2 && *v == 1) || (*h == 2 && *v == 2)))
    return fail(MDCT_INVALID_PARAMETER, "luma sampling factors %dx%d (1x1, 2x1 or 2x2)", *h, *v);
  *mcus_x = planes[1].blocks_x;
  *mcus_y = planes[1].blocks_y;
  for (int c = 0; c < 3; c++)
  {
    const mdct_jpegcoef_plane &p = planes[c];
    if ((uint64_t)p.blocks_x != (uint64_t)*mcus_x * (uint32_t)p.h || (uint64_t)p.blocks_y != (uint64_t)*mcus_y * (uint32_t)p.v)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: %u x %u blocks at sampling %dx%d is not on the MCU grid of %u x %u MCUs the chroma planes state (blocks_x = "
                  "mcus_x * h, blocks_y = mcus_y * v)", c, p.blocks_x, p.blocks_y, p.h, p.v, *mcus_x, *mcus_y);
  }
  return MDCT_SUCCESS;
}

[[maybe_unused]] int check_word(const void *p, const char *name)
{
  if ((uintptr_t)p & 3)
    return fail(MDCT_INVALID_PARAMETER, "%s is not 4-byte aligned", name);
  return MDCT_SUCCESS;
}

} // namespace
