/* mdct_jpegenc_scan.h -- C-ABI of libmdct_jpegenc_scan.so: the three component planes of a colour JPEG encode -> the Huffman
 * segments of ONE INTERLEAVED scan (ITU-T T.81 A.2.3), one segment per MCU row, on the GPU.
 *
 * A separate library, linked against libmdct_hip.so (include/mdct.h), whose status codes, launch tally, Huffman specifications and
 * packing call it uses.  Pointers are device pointers unless stated; `stream` is a hipStream_t passed as void* (NULL = the null
 * stream).  The call is one asynchronous launch on that stream; nothing is allocated or synchronised inside (safe for hipGraph
 * capture).  Every argument is checked on the host before the device is touched: MDCT_INVALID_PARAMETER with detail in
 * mdct_jpegenc_scan_last_error().
 */
#ifndef MDCT_JPEGENC_SCAN_H
#define MDCT_JPEGENC_SCAN_H

#include <stddef.h>
#include <stdint.h>

#include "mdct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One component plane as mdct_jpegenc_from_rgb (include/mdct_jpegenc.h) leaves it, PADDED TO THE MCU GRID:
 * width = mcus_x * 8 * h, height = mcus_y * 8 * v (at most 65536 each); pitch in bytes, >= width, no alignment requirement on px
 * or pitch. */
typedef struct
{
  const uint8_t *px;
  size_t pitch;
  size_t width, height;
  int h, v; /* sampling factors */
} mdct_jpegenc_scan_plane;

/* planes: Y, Cb, Cr (n_planes = 3) with sampling (2,2)/(1,1)/(1,1), (2,1)/(1,1)/(1,1) or (1,1)/(1,1)/(1,1); anything else is
 * refused, and so are planes that do not describe the same mcus_x x mcus_y grid.
 * lut_luma / lut_chroma: HOST pointers to 64 floats, natural order v*8+u, finite and non-zero, as for mdct_fwd_u8_huffman_rows; the
 * level shift is always on.  Block for block the coded coefficients are what mdct_fwd_u8_i16 gives for that plane and table, AC
 * levels saturated to +-1023.
 * MCU rows my0 <= my < my1 are coded, one workgroup and one segment each: the segment of MCU row my starts at out + my * seg_stride
 * and holds a restart interval of mcus_x MCUs, blocks in the order of T.81 A.2.3 (4:2:0: Y00 Y01 Y10 Y11 Cb Cr), every component with
 * its own DC predictor (0 at the start of the segment), the Annex K tables (luminance for Y, chrominance for Cb and Cr); byte-aligned,
 * the last byte padded with 1-bits, NOT stuffed.  seg_bytes[my] = its length, ff_counts[my] = the number of 0xFF bytes in it:
 * exactly the segment contract of mdct_fwd_u8_huffman_rows, so
 *     mdct_jpeg_pack_rows_counted(out, seg_bytes, ff_counts, seg_stride, mcus_y, 0, scan, capacity, row_offsets, stream)
 * finishes the scan (DRI = mcus_x).
 * seg_stride: a multiple of 4, >= mdct_jpegenc_scan_seg_stride(mcus_x, blocks per MCU); out 4-byte aligned. */
int mdct_jpegenc_scan_rows(const mdct_jpegenc_scan_plane *planes, int n_planes, const float *lut_luma, const float *lut_chroma,
                           size_t my0, size_t my1, uint8_t *out, size_t seg_stride, uint32_t *seg_bytes, uint32_t *ff_counts, void *stream);

/* smallest legal seg_stride: 208 * (mcus_x * blocks_per_mcu) + 8 (host function) */
size_t mdct_jpegenc_scan_seg_stride(size_t mcus_x, int blocks_per_mcu);

/* detail of the last failure of this library on any thread (host function) */
const char *mdct_jpegenc_scan_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
