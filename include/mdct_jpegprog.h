/* mdct_jpegprog.h -- C-ABI of libmdct_jpegprog.so: the scans of a progressive JPEG (SOF2) with spectral selection, Ah = Al = 0
 * (ITU-T T.81 Annex G.1.2), coded from quantised coefficient planes: one DC scan, then scans of one band Ss..Se of one component with
 * end-of-band runs.  Successive approximation (refinement scans) is out of scope.  libmdct_jpegdec_prog.so
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

/* detail of the last failure of this library on any thread (host function) */
const char *mdct_jpegprog_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
