/* mdct_jpegcolor.h -- C-ABI of libmdct_jpegcolor.so: decoded JPEG component planes -> an 8-bit RGB image on the GPU.
 *
 * The last stage of a JPEG decode (include/mdct_jpegdec.h leaves one plane per component): chroma upsampling and YCbCr -> RGB, bit
 * for bit as libjpeg-turbo's default decompression gives them ("fancy" upsampling, integer colour tables).
 * Each component is given at its true size, ceil(W * h / hmax) x ceil(H * v / vmax): the padding of an MCU-aligned plane is not read,
 * the component's own last column and row stand in for it.  Every ratio hmax / h and vmax / v must be a whole number 1..4.
 *
 * Nothing is allocated or synchronised inside mdct_jpegcolor_to_rgb and it is one kernel launch: it may be captured into a hipGraph.
 * Return codes are those of include/mdct.h; the message of this library's last failure is mdct_jpegcolor_last_error().  The library
 * links against libmdct_hip.so; its launches appear in mdct_kernel_counts(). */
#ifndef MDCT_JPEGCOLOR_H
#define MDCT_JPEGCOLOR_H

#include <stddef.h>
#include <stdint.h>

#include "mdct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* colour spaces of the planes */
#define MDCT_JPEGCOLOR_YCBCR 0 /* three planes Y, Cb, Cr: upsampled, then converted */
#define MDCT_JPEGCOLOR_RGB 1   /* three planes R, G, B (Adobe transform 0): upsampled, not converted */
#define MDCT_JPEGCOLOR_GREY 2  /* one plane, copied into all three channels */

/* layouts of the output */
#define MDCT_JPEGCOLOR_HWC 0 /* rows of W interleaved R, G, B byte triples, out_pitch bytes apart */
#define MDCT_JPEGCOLOR_CHW 1 /* three planes R, G, B, out_plane_stride bytes apart, each H rows of W bytes, out_pitch bytes apart */

typedef struct
{
  const uint8_t *px; /* device pointer to the component's first sample */
  size_t pitch;      /* bytes between rows, >= width */
  size_t width;      /* true size of the component */
  size_t height;
  int h, v;          /* sampling factors of the frame header, 1..4 */
} mdct_jpegcolor_plane;

/* planes -> RGB in out.  n_planes: 1 (GREY) or 3 (YCBCR, RGB); width, height: the image, 1..65535.  Nothing outside the H rows x 3W
 * bytes (HWC) or the three H x W planes (CHW) of out is written, and out must not overlap any input plane.  Offsets are 64-bit.
 * Invalid arguments are refused on the host, without touching the device (MDCT_INVALID_PARAMETER, message set). */
int mdct_jpegcolor_to_rgb(const mdct_jpegcolor_plane *planes, int n_planes, size_t width, size_t height, int colour, int layout,
                          uint8_t *out, size_t out_pitch, size_t out_plane_stride, void *stream);

/* message of this library's last failure */
const char *mdct_jpegcolor_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MDCT_JPEGCOLOR_H */
