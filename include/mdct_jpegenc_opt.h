/* mdct_jpegenc_opt.h -- C-ABI of libmdct_jpegenc_opt.so: JPEG encoding with Huffman tables made for the image (ITU-T T.81 K.2,
 * libjpeg's optimize_coding): the symbol statistics of the planes about to be coded, the tables for those statistics, and coders
 * that take the caller's tables instead of the Annex K ones.
 *
 * A separate library, linked against libmdct_hip.so (include/mdct.h), whose status codes, launch tally and packing call it uses.
 * Pointers are device pointers unless stated; `stream` is a hipStream_t passed as void* (NULL = the null stream).  The device calls are
 * asynchronous on that stream; nothing is allocated or synchronised inside (safe for hipGraph capture).  Every argument is checked on
 * the host before the device is touched: MDCT_INVALID_PARAMETER with detail in mdct_jpegenc_opt_last_error().
 */
#ifndef MDCT_JPEGENC_OPT_H
#define MDCT_JPEGENC_OPT_H

#include <stddef.h>
#include <stdint.h>

#include "mdct.h"
#include "mdct_jpegenc_scan.h" /* mdct_jpegenc_scan_plane */

#ifdef __cplusplus
extern "C" {
#endif

#define MDCT_JPEGENC_OPT_HIST_CLASS 272 /* counts per class: 16 DC categories, then the 256 AC symbols RRRRSSSS */

/* A Huffman specification as a DHT segment carries it (HOST pointers): 16 counts of codes per length, then the symbols in code order. */
typedef struct
{
  const uint8_t *bits16;
  const uint8_t *vals;
  int nvals;
} mdct_jpegenc_opt_spec;

/* Symbol statistics: hist is uint32_t[2][272], class 0 luminance (plane 0), class 1 chrominance (planes 1 and 2 summed); entries 0..15
 * of a class count the DC categories (0..11 occur), entries 16 + RRRRSSSS the AC symbols, ZRL (0xF0) and EOB (0x00) included.  The call
 * zeroes hist itself (a memset node on the stream) and then counts: afterwards hist holds the counts of this call alone.
 * Counted are exactly the symbols the coder of the same planes and tables emits: the coefficients of mdct_fwd_u8_i16 with the level
 * shift, AC levels saturated to +-1023, DC differences to +-2047, a ZRL per 16 zeros before a level, EOB unless index 63 is coded,
 * the DC predictor 0 at the start of every restart interval.  The intervals depend on the scan form:
 *   interleaved = 0   every plane is a scan of its own over its own block grid, interval = one block row (mdct_jpegenc_opt_rows,
 *                     mdct_fwd_u8_huffman_rows).  n_planes 1 or 3; width and height multiples of 8 (8..65536), pitch >= width; h and v
 *                     are not read.  One launch per plane.
 *   interleaved = 1   the MCU order of T.81 A.2.3, interval = one MCU row (mdct_jpegenc_opt_scan_rows, mdct_jpegenc_scan_rows): three
 *                     planes on the MCU grid with the samplings that call takes.  One plane: as interleaved = 0.  One launch.
 * lut_luma / lut_chroma: HOST pointers to 64 floats, natural order v*8+u, finite and non-zero (lut_chroma is not read for one plane). */
int mdct_jpegenc_opt_stats(const mdct_jpegenc_scan_plane *planes, int n_planes, const float *lut_luma, const float *lut_chroma, int interleaved,
                           uint32_t *hist, void *stream);

/* The optimal table for the counts of one class (host function, all pointers HOST): libjpeg's jpeg_gen_optimal_table, that is T.81 K.2
 * with a 257th symbol of frequency 1 so that no symbol gets the all-ones code, ties resolved towards the larger symbol, Figure K.3's
 * adjustment down to 16 bits, the reserved symbol taken from the longest length in use, the symbols ordered by code length, then value.
 * Symbols with count 0 get no code.  n_symbols: 12..16 for a DC class, 256 for an AC class; vals takes up to n_symbols bytes.
 * (Code lengths beyond 32 before the adjustment, which libjpeg refuses, go through the same adjustment.)  Counts that are all zero are
 * refused. */
int mdct_jpegenc_opt_table(const uint32_t *counts, int n_symbols, uint8_t bits16[16], uint8_t *vals, int *nvals);

/* One plane -> one Huffman segment per block row, as mdct_fwd_u8_huffman_rows (level shift on, lut required: HOST pointer, 64 floats)
 * with the caller's DC and AC specification in place of `chroma`.  Same segment contract: block row by at out + by * seg_stride,
 * byte-aligned, padded with 1-bits, NOT stuffed, seg_bytes[by] its length and ff_counts[by] its 0xFF bytes, so
 * mdct_jpeg_pack_rows_counted finishes the scan.  What differs from the Annex K coders:
 *   worst case   with any legal table a block takes up to 16 + 11 bits of DC and 63 * (16 + 10) of AC = 1665 bits, more than the 208
 *                bytes per block of mdct_huffman_seg_stride: seg_stride must be a multiple of 4 and
 *                >= mdct_jpegenc_opt_seg_stride(sizeX / 8).
 *   uncoded      a specification is checked as mdct_jpegdec_tables_check checks one (counts and values agree, 1..256 values, baseline
 *                symbols, not over-subscribed, no all-ones code) and may not name a symbol twice.  It need not cover the plane: a symbol
 *                that occurs and has no code is coded as its amplitude bits alone (the segment stays within the worst case and is not
 *                decodable) and counted: *uncoded, a device word the CALLER zeroes, is increased by the number of such symbols.  Tables
 *                made from mdct_jpegenc_opt_stats of the same planes and luts leave it 0. */
int mdct_jpegenc_opt_rows(const uint8_t *px, size_t pitch, const float *lut, size_t sizeX, size_t sizeY, size_t by0, size_t by1,
                          const mdct_jpegenc_opt_spec *dc, const mdct_jpegenc_opt_spec *ac, uint8_t *out, size_t seg_stride, uint32_t *seg_bytes,
                          uint32_t *ff_counts, uint32_t *uncoded, void *stream);

/* Three planes -> the segments of one interleaved scan, as mdct_jpegenc_scan_rows (include/mdct_jpegenc_scan.h) with the caller's
 * specifications: specs[0] DC luminance, [1] AC luminance, [2] DC chrominance, [3] AC chrominance (the order of mdct_huffman_spec).
 * seg_stride: a multiple of 4, >= mdct_jpegenc_opt_seg_stride(mcus_x * blocks per MCU); uncoded as above. */
int mdct_jpegenc_opt_scan_rows(const mdct_jpegenc_scan_plane *planes, int n_planes, const float *lut_luma, const float *lut_chroma,
                               const mdct_jpegenc_opt_spec specs[4], size_t my0, size_t my1, uint8_t *out, size_t seg_stride, uint32_t *seg_bytes,
                               uint32_t *ff_counts, uint32_t *uncoded, void *stream);

/* smallest legal seg_stride for `blocks` blocks per segment: 209 * blocks + 8, rounded up to a multiple of 4 (host function) */
size_t mdct_jpegenc_opt_seg_stride(size_t blocks);

/* detail of the last failure of this library on any thread (host function) */
const char *mdct_jpegenc_opt_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
