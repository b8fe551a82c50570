/* mdct_jpegscale.h -- C-ABI of libmdct_jpegscale.so: quantised JPEG coefficient planes -> 8-bit planes at 1/2, 1/4 or 1/8 size.
 *
 * The reduced-size inverse of a JPEG decode (libjpeg's scale_denom).  A block decoded to n x n samples,
 * n = 4, 2 or 1, holds the mean over each (8/n) x (8/n) group of the mathematical 8x8 IDCT of its dequantised coefficients:
 *   out = clamp(rne(boxmean(IDCT(c * Q)) + 128 * level_shift), 0, 255)
 * as libjpeg-turbo's jidctred.c defines it (not the low-frequency truncation of libjpeg 7 and later).  n = 8 is not taken: the full
 * inverse is mdct_inv_i16_u8_batch (include/mdct.h).
 *
 * Nothing is allocated or synchronised inside mdct_jpegscale_inv_i16_u8 and it is one kernel launch for all planes: it may be captured
 * into a hipGraph.  Descriptors and tables travel in the kernel arguments.  Return codes are those of include/mdct.h; the message of
 * this library's last failure is mdct_jpegscale_last_error().  The library links against libmdct_hip.so; its launches appear in
 * mdct_kernel_counts(). */
#ifndef MDCT_JPEGSCALE_H
#define MDCT_JPEGSCALE_H

#include <stddef.h>
#include <stdint.h>

#include "mdct.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct
{
  const int16_t *coef; /* device: blocks_y * 8 rows of blocks_x * 8 coefficients in natural order, as mdct_fwd_u8_i16 writes them */
  size_t pitch_coef;   /* elements between rows, >= blocks_x * 8; rows 16-byte aligned (coef aligned, pitch_coef a multiple of 8) */
  uint8_t *px;         /* device: blocks_y * n rows of blocks_x * n samples; no alignment requirement */
  size_t pitch_px;     /* bytes between rows, >= blocks_x * n */
  size_t blocks_x, blocks_y; /* 1..8192 each */
  const float *lut;    /* HOST: the quantisation table, 64 floats in natural order (v * 8 + u), finite and non-zero; NULL: all ones */
  int n;               /* output samples per block side: 4, 2 or 1 */
  int rep_x, rep_y;    /* n = 1 only: every sample is written rep_x x rep_y times (1..4; 0 means 1), the plane is then
                          blocks_y * rep_y rows of blocks_x * rep_x bytes.  libjpeg upsamples by plain replication at 1/8 */
} mdct_jpegscale_plane;

/* n_planes: 1..4, of any mix of n.  level_shift: 0 or 1 (adds 128).  Nothing outside each plane's blocks_y * n rows of blocks_x * n
 * bytes (times rep_y, rep_x) is written; no output may overlap any plane's coefficients.  Invalid arguments are refused on the host, without touching the
 * device (MDCT_INVALID_PARAMETER, message set). */
int mdct_jpegscale_inv_i16_u8(const mdct_jpegscale_plane *planes, int n_planes, int level_shift, void *stream);

/* message of this library's last failure */
const char *mdct_jpegscale_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MDCT_JPEGSCALE_H */
