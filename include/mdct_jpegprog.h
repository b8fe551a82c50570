/* mdct_jpegprog.h -- C-ABI of libmdct_jpegprog.so: the scans of a progressive JPEG (SOF2), spectral selection and successive
 * approximation (ITU-T T.81 Annex G.1.2), coded from quantised coefficient planes: DC scans, and scans of one band Ss..Se of one
 * component with end-of-band runs; first scans and refinement scans (the ..._approx calls below).  libmdct_jpegdec_prog.so
 * (include/mdct_jpegdec_prog.h) decodes these scans back into the planes.
 *
 * A separate library, linked against libmdct_hip.so (include/mdct.h: status codes, launch tally, the packing call) and
 * libmdct_jpegenc_opt.so (include/mdct_jpegenc_opt.h: the specification type, the segment stride, the table maker, which takes the
 * counts of EOBn symbols like any others).  Planes are mdct_jpegcoef_plane (include/mdct_jpegcoef.h), the contract unchanged.
 * Pointers are device pointers unless stated; `stream` is a hipStream_t passed as void* (NULL = the null stream).  The device calls
 * are asynchronous on that stream; nothing is allocated or synchronised inside (safe for hipGraph capture).  Every argument is checked
 * on the host before the device is touched: MDCT_INVALID_PARAMETER with detail in mdct_jpegprog_last_error().
 *
 * Segments follow the contract of mdct_jpegenc_opt_rows: interval r at out + r * seg_stride, byte-aligned, padded with 1-bits, NOT
 * stuffed, seg_bytes[r] its length and ff_counts[r] its 0xFF bytes, so mdct_jpeg_pack_rows_counted finishes the scan.
 *
 * seg_stride: a multiple of 4, >= mdct_jpegenc_opt_seg_stride(blocks per interval) = 209 * blocks + 8, rounded up to 4.  That stride
 * holds here: a DC-first block is at most 16 + 11 bits.  A block of an AC band is at most 63 levels of 16 + 10 bits (a ZRL, 16 bits,
 * stands for 16 of them and is shorter) = 1638 bits, after at most one end-of-band run token flushed in front of it, 16 + 14 bits:
 * 1668 bits against the 1672 of 209 bytes; a block without levels adds at most that one token.  The run flushed at the end of an
 * interval (30 bits) and the padded last dword fit in the 8 bytes.
 */
#ifndef MDCT_JPEGPROG_H
#define MDCT_JPEGPROG_H

#include <stddef.h>
#include <stdint.h>

#include "mdct.h"
#include "mdct_jpegcoef.h"    /* mdct_jpegcoef_plane */
#include "mdct_jpegenc_opt.h" /* mdct_jpegenc_opt_spec, mdct_jpegenc_opt_seg_stride, MDCT_JPEGENC_OPT_HIST_CLASS */

#ifdef __cplusplus
extern "C" {
#endif

/* The DC-first scan (G.1.2.1 with Al = 0): per block the DC difference alone, category code plus amplitude bits, no EOB; the predictor
 * is 0 at the start of every interval.
 *   interleaved = 0   ONE plane (n_planes = 1), an interval per block row.
 *   interleaved = 1   three planes in MCU order with the samplings mdct_jpegcoef_scan_rows takes, an interval per MCU row.
 * hist: uint32_t[2][272], zeroed by the call itself; only entries 0..15 of a class are used, class 0 for plane 0 (cls = 0) and class
 * 1 for the chroma planes (or the one plane with cls = 1).  A DC difference outside +-2047 is clamped and counted in *unrepresentable,
 * a device word the CALLER zeroes. */
int mdct_jpegprog_dc_stats(const mdct_jpegcoef_plane *planes, int n_planes, int interleaved, int cls, uint32_t *hist, uint32_t *unrepresentable, void *stream);

/* Intervals r0 .. r1 - 1 (block rows, or MCU rows of the interleaved form) of the DC scan.  specs: one specification (one plane) or two
 * (luminance, chrominance), validated as mdct_jpegcoef_rows validates a DC specification.  uncoded: a device word the caller zeroes,
 * increased by the number of symbols the tables have no code for. */
int mdct_jpegprog_dc_rows(const mdct_jpegcoef_plane *planes, int n_planes, int interleaved, const mdct_jpegenc_opt_spec *specs, size_t r0, size_t r1, uint8_t *out,
                          size_t seg_stride, uint32_t *seg_bytes, uint32_t *ff_counts, uint32_t *uncoded, uint32_t *unrepresentable, void *stream);

/* One AC band ss..se (1 <= ss <= se <= 63, zig-zag positions) of ONE plane (G.1.2.2 with Al = 0; AC scans are never interleaved,
 * G.1.1.1.1), an interval per block row, exactly libjpeg's encode_mcu_AC_first: within a block a non-zero level first flushes the
 * pending end-of-band run, then emits one ZRL (0xF0) per 16 zeros since the last coded position INSIDE the band, then RRRRSSSS and
 * the amplitude bits; a block whose position se is zero adds 1 to the run; a run of 0x7FFF is emitted at once; a run is the symbol
 * n << 4, n = floor(log2(run)), followed by the low n bits of the run; the run is flushed at the end of every interval.
 * hist: uint32_t[256] by RRRRSSSS, zeroed by the call itself: exactly the symbols the coder emits, EOB0 .. EOB14 (0x00 .. 0xE0)
 * included.  An AC level of the band outside +-1023 is clamped and counted in *unrepresentable (caller-zeroed). */
int mdct_jpegprog_ac_stats(const mdct_jpegcoef_plane *plane, int ss, int se, uint32_t *hist, uint32_t *unrepresentable, void *stream);

/* Block rows by0 .. by1 - 1 of the band's scan.  ac: validated as mdct_jpegcoef_rows validates an AC specification (the symbols
 * 0x10 .. 0xE0 are the EOBn of this scan).  uncoded as above. */
int mdct_jpegprog_ac_rows(const mdct_jpegcoef_plane *plane, int ss, int se, size_t by0, size_t by1, const mdct_jpegenc_opt_spec *ac, uint8_t *out, size_t seg_stride,
                          uint32_t *seg_bytes, uint32_t *ff_counts, uint32_t *uncoded, uint32_t *unrepresentable, void *stream);

/* Successive approximation (G.1.2): the four calls above with the scan's Ah and Al; with ah = al = 0 they write what those write.
 * Refused on the host (MDCT_INVALID_PARAMETER): al outside 0..13, and ah not in {0, al + 1}.
 *
 * DC first, al > 0 (encode_mcu_DC_first): the differences of dc >> al, an arithmetic shift; differences of the shifted values outside
 * +-2047 are counted as above.
 * DC refinement, ah = al + 1 (dc_rows_approx only; dc_stats_approx refuses ah != 0, there are no symbols): one raw bit
 * (dc >> al) & 1 per block in scan order, padded with 1-bits; no table (specs may be NULL), nothing is added to *uncoded or
 * *unrepresentable.  One plane with an interval per block row, or three in MCU order with an interval per MCU row, as the first scan.
 *
 * AC first, al > 0 (encode_mcu_AC_first): the level is |v| >> al with v's sign; a level that becomes 0 counts as a zero, for runs and
 * for the tail flag alike.
 * AC refinement, ah = al + 1 (encode_mcu_AC_refine, exactly).  Let a[k] = |v[k]| >> al and EOB the last k of the band with a[k] == 1.
 * Walking k = ss..se: a == 0 counts a zero, r++.  At a non-zero position, first: while r > 15 and k <= EOB, flush the pending run
 * with its buffered bits, emit ZRL and then the block's buffered correction bits, r -= 16.  a > 1: buffer the correction bit a & 1.
 * a == 1: flush the pending run with its bits, emit (r << 4) | 1, a sign bit (1: positive) and the block's buffered correction bits;
 * r = 0.  After the block: if r > 0 or bits are buffered, the run grows by one and takes the block's bits; it is flushed at once when
 * it reaches 0x7FFF or holds more than 937 bits, and at the end of every interval.  A flush emits EOBn (none for a run of 0), its n
 * extra bits, then the buffered bits in order.  hist: exactly the symbols emitted.
 *
 * Clamping: an AC level is clamped to +-1023 BEFORE the point transform in every AC scan kind, so all scans of one coefficient agree;
 * a clamped level is counted in *unrepresentable by the first scan of its band only (ah = 0), never by a refinement scan.
 *
 * seg_stride: mdct_jpegenc_opt_seg_stride still bounds a segment.  DC scans: at most 27 bits, or one bit, per block.  AC refinement:
 * charge every bit to the block whose coefficient it codes, buffered or not.  A position of the band gives its block at most 17 bits
 * -- a == 1: a code of at most 16 bits and the sign bit; a > 1: one correction bit; a == 0: at most 1/16 of a ZRL of 16 bits -- so a
 * block owns at most 63 * 17 = 1071 bits wherever in the segment they end up.  Every EOBn token (at most 16 + 14 bits) is emitted
 * for a run that begins at some tail block, and a block begins at most one run: charged to that block, 1101 bits in all, below the
 * 1672 of 209 bytes.  Nothing is emitted that is charged to no block, so an interval of n blocks holds at most 1101 n bits; the
 * padded last dword fits in the 8 bytes.  An AC first scan with al > 0 emits the symbols of an al = 0 scan of the shifted levels. */
int mdct_jpegprog_dc_stats_approx(const mdct_jpegcoef_plane *planes, int n_planes, int interleaved, int cls, int ah, int al, uint32_t *hist, uint32_t *unrepresentable,
                                  void *stream);
int mdct_jpegprog_dc_rows_approx(const mdct_jpegcoef_plane *planes, int n_planes, int interleaved, const mdct_jpegenc_opt_spec *specs, int ah, int al, size_t r0, size_t r1,
                                 uint8_t *out, size_t seg_stride, uint32_t *seg_bytes, uint32_t *ff_counts, uint32_t *uncoded, uint32_t *unrepresentable, void *stream);
int mdct_jpegprog_ac_stats_approx(const mdct_jpegcoef_plane *plane, int ss, int se, int ah, int al, uint32_t *hist, uint32_t *unrepresentable, void *stream);
int mdct_jpegprog_ac_rows_approx(const mdct_jpegcoef_plane *plane, int ss, int se, int ah, int al, size_t by0, size_t by1, const mdct_jpegenc_opt_spec *ac, uint8_t *out,
                                 size_t seg_stride, uint32_t *seg_bytes, uint32_t *ff_counts, uint32_t *uncoded, uint32_t *unrepresentable, void *stream);

/* detail of the last failure of this library on any thread (host function) */
const char *mdct_jpegprog_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
