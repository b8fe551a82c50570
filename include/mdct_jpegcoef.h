/* mdct_jpegcoef.h -- C-ABI of libmdct_jpegcoef.so: JPEG in the coefficient domain.  The quantised coefficient planes a decode leaves
 * (mdct_jpegdec_decode, include/mdct_jpegdec.h) are coded again -- with any Huffman tables, in either scan form -- or flipped, transposed
 * and rotated by quarter turns, without an inverse or forward DCT and so without a second quantisation: what jpegtran does.
 *
 * A separate library, linked against libmdct_hip.so (include/mdct.h: status codes, launch tally, the packing call) and
 * libmdct_jpegenc_opt.so (include/mdct_jpegenc_opt.h: the specification type and the segment stride).  Pointers are device pointers
 * unless stated; `stream` is a hipStream_t passed as void* (NULL = the null stream).  The device calls are asynchronous on that stream;
 * nothing is allocated or synchronised inside (safe for hipGraph capture).  Every argument is checked on the host before the device is
 * touched: MDCT_INVALID_PARAMETER with detail in mdct_jpegcoef_last_error().
 */
#ifndef MDCT_JPEGCOEF_H
#define MDCT_JPEGCOEF_H

#include <stddef.h>
#include <stdint.h>

#include "mdct.h"
#include "mdct_jpegenc_opt.h" /* mdct_jpegenc_opt_spec, mdct_jpegenc_opt_seg_stride, MDCT_JPEGENC_OPT_HIST_CLASS */

#ifdef __cplusplus
extern "C" {
#endif

/* A coefficient plane in the layout mdct_jpegdec_decode writes: level (v, u) of block (by, bx) at row by * 8 + v, column bx * 8 + u,
 * quantised (not dequantised).  pitch: int16 elements between rows, a multiple of 8 and >= blocks_x * 8; coef 16-byte aligned (so every
 * row of every block is).  blocks_x, blocks_y: 1..65535, the blocks a call works on -- stated apart from the allocation, so a caller
 * may code fewer blocks than the plane holds (a component's own block grid inside a plane padded to the MCU grid).  h, v: the sampling
 * factors, read by the interleaved forms only. */
typedef struct
{
  int16_t *coef;
  size_t pitch;
  uint32_t blocks_x, blocks_y;
  int h, v;
} mdct_jpegcoef_plane;

/* Symbol statistics, the histogram contract of mdct_jpegenc_opt_stats: hist is uint32_t[2][272], zeroed by the call itself, class 0 for
 * plane 0 and class 1 for the others; counted are exactly the symbols the coders below emit for these planes.
 *   interleaved = 0   every plane is a scan of its own over blocks_x x blocks_y, one interval per block row (mdct_jpegcoef_rows).
 *                     n_planes 1 or 3.  One launch per plane.
 *   interleaved = 1   three planes on one MCU grid, luma sampling (2,2), (2,1) or (1,1), chroma (1,1), plane c holding
 *                     mcus_x * h x mcus_y * v blocks; one interval per MCU row (mdct_jpegcoef_scan_rows).  One plane: as 0.  One launch.
 * unrepresentable: as for the coders (the same events, counted once more). */
int mdct_jpegcoef_stats(const mdct_jpegcoef_plane *planes, int n_planes, int interleaved, uint32_t *hist, uint32_t *unrepresentable, void *stream);

/* One plane -> one Huffman segment per block row by0 .. by1 - 1, the segment contract of mdct_jpegenc_opt_rows: block row by at
 * out + by * seg_stride, byte-aligned, padded with 1-bits, NOT stuffed, seg_bytes[by] its length and ff_counts[by] its 0xFF bytes, so
 * mdct_jpeg_pack_rows_counted finishes the scan.  seg_stride: a multiple of 4, >= mdct_jpegenc_opt_seg_stride(blocks_x).  dc / ac: the
 * caller's specifications, validated as mdct_jpegenc_opt_rows validates them, with the same `uncoded` rule.
 * Loss is never silent: an AC level outside +-1023 or a DC difference outside +-2047 cannot be written in a baseline scan.  Such a
 * value is clamped (the segment stays inside its worst case) and counted: *unrepresentable, a device word the CALLER zeroes, is
 * increased by the number of such values. */
int mdct_jpegcoef_rows(const mdct_jpegcoef_plane *plane, size_t by0, size_t by1, const mdct_jpegenc_opt_spec *dc, const mdct_jpegenc_opt_spec *ac, uint8_t *out,
                       size_t seg_stride, uint32_t *seg_bytes, uint32_t *ff_counts, uint32_t *uncoded, uint32_t *unrepresentable, void *stream);

/* Three planes -> the segments of one interleaved scan (T.81 A.2.3), MCU rows my0 .. my1 - 1, the segment contract of
 * mdct_jpegenc_opt_scan_rows: specs[0] DC luminance, [1] AC luminance, [2] DC chrominance, [3] AC chrominance; seg_stride a multiple of
 * 4, >= mdct_jpegenc_opt_seg_stride(mcus_x * blocks per MCU).  uncoded and unrepresentable as above. */
int mdct_jpegcoef_scan_rows(const mdct_jpegcoef_plane *planes, int n_planes, const mdct_jpegenc_opt_spec specs[4], size_t my0, size_t my1, uint8_t *out,
                            size_t seg_stride, uint32_t *seg_bytes, uint32_t *ff_counts, uint32_t *uncoded, uint32_t *unrepresentable, void *stream);

/* The lossless geometric operations on a coefficient plane: a permutation of blocks, a transposition inside each block and sign
 * changes.  With BX x BY the blocks of src:
 *   FLIP_H      block (by, bx) -> (by, BX - 1 - bx), c'[v][u] = (-1)^u c[v][u]
 *   FLIP_V      block (by, bx) -> (BY - 1 - by, bx), c'[v][u] = (-1)^v c[v][u]
 *   TRANSPOSE   block (by, bx) -> (bx, by),          c'[v][u] = c[u][v]
 *   ROT180 = FLIP_H o FLIP_V;  ROT90 (clockwise) = TRANSPOSE, then FLIP_H;  ROT270 = FLIP_H, then TRANSPOSE;
 *   TRANSVERSE = TRANSPOSE, then ROT180.
 * The caller transposes the quantisation table with the four transposing operations. */
enum
{
  MDCT_JPEGCOEF_FLIP_H = 0,
  MDCT_JPEGCOEF_FLIP_V = 1,
  MDCT_JPEGCOEF_TRANSPOSE = 2,
  MDCT_JPEGCOEF_TRANSVERSE = 3,
  MDCT_JPEGCOEF_ROT90 = 4,
  MDCT_JPEGCOEF_ROT180 = 5,
  MDCT_JPEGCOEF_ROT270 = 6
};

/* src's blocks_x x blocks_y blocks -> dst, which states the same grid, or the swapped grid for the four transposing operations
 * (anything else is refused); planes whose bytes overlap are refused.  h and v are not read.  The negation of -32768 wraps. */
int mdct_jpegcoef_transform(const mdct_jpegcoef_plane *src, const mdct_jpegcoef_plane *dst, int op, void *stream);

/* detail of the last failure of this library on any thread (host function) */
const char *mdct_jpegcoef_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
