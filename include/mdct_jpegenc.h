/* mdct_jpegenc.h -- C-ABI of libmdct_jpegenc.so: an 8-bit RGB or grey image -> the padded component planes of a baseline JPEG encode.
 *
 * The first stage of a JPEG encode, the mirror of include/mdct_jpegcolor.h: RGB -> YCbCr, chroma downsampling and edge padding to
 * the block grid, bit for bit as libjpeg-turbo's compressor gives them (jccolor.c rgb_ycc_convert, jcsample.c).
 * The planes then go through the scan kernels of include/mdct.h (mdct_fwd_u8_jpeg_scan, one non-interleaved scan per component).
 *
 * The rules, for pixels R, G, B (0..255) and arithmetic shifts:
 *   Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + (128 << 16) + 32767) >> 16
 *   Cr = (32768 R - 27439 G - 5329 B + (128 << 16) + 32767) >> 16
 *   4:2:2 (chroma 2x1 of luma): c[x] = (p[2x] + p[2x+1] + bias) >> 1,                 bias 0, 1, 0, 1 ... by output column x
 *   4:2:0 (chroma 2x2 of luma): c[x] = (the 2x2 group p[2x..2x+1][2y..2y+1] + bias) >> 2, bias 1, 2, 1, 2 ... by output column x
 *   A component's true size is ceil(W * h / hmax) x ceil(H * v / vmax).  Inside it, a group that reaches past the image takes the
 *   image's last column (row) in place of the missing ones (libjpeg's expand_right_edge and bottom-edge row-group fill).
 *   Beyond it, up to the plane's padded size, every sample repeats the component's own last true column and row.
 * Grey images are copied, with the same padding.
 *
 * Nothing is allocated or synchronised inside mdct_jpegenc_from_rgb and it is one kernel launch: it may be captured into a hipGraph.
 * Return codes are those of include/mdct.h; the message of this library's last failure is mdct_jpegenc_last_error().  The library
 * links against libmdct_hip.so; its launches appear in mdct_kernel_counts(). */
#ifndef MDCT_JPEGENC_H
#define MDCT_JPEGENC_H

#include <stddef.h>
#include <stdint.h>

#include "mdct.h"

#ifdef __cplusplus
extern "C" {
#endif

/* colour of the input */
#define MDCT_JPEGENC_RGB 0  /* three channels R, G, B -> three planes Y, Cb, Cr */
#define MDCT_JPEGENC_GREY 1 /* one channel -> one plane; the layout is ignored */

/* layouts of an RGB input */
#define MDCT_JPEGENC_HWC 0 /* rows of W interleaved R, G, B byte triples, in_pitch bytes apart */
#define MDCT_JPEGENC_CHW 1 /* three planes R, G, B, in_plane_stride bytes apart, each H rows of W bytes, in_pitch bytes apart */

typedef struct
{
  uint8_t *px;       /* device pointer to the plane's first sample */
  size_t pitch;      /* bytes between rows, >= width */
  size_t width;      /* padded size of the plane: multiples of 8, at least the component's true size, at most 65536 */
  size_t height;
  int h, v;          /* sampling factors of the frame header */
} mdct_jpegenc_plane;

/* image -> planes.  width, height: the image, 1..65535.  colour GREY: one plane, (h, v) = (1, 1).  colour RGB: three planes Y, Cb, Cr
 * with (h, v) = (1,1) / (1,1) / (1,1) (4:4:4), (2,1) / (1,1) / (1,1) (4:2:2) or (2,2) / (1,1) / (1,1) (4:2:0); every other mix is
 * refused.  Every byte of each plane's height rows x width columns is written and nothing else; no output plane may overlap the input
 * or another output plane.  Offsets are 64-bit.  Invalid arguments are refused on the host, without touching the device
 * (MDCT_INVALID_PARAMETER, message set). */
int mdct_jpegenc_from_rgb(const uint8_t *in, size_t in_pitch, size_t in_plane_stride, size_t width, size_t height, int colour, int layout,
                          const mdct_jpegenc_plane *planes, int n_planes, void *stream);

/* message of this library's last failure */
const char *mdct_jpegenc_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MDCT_JPEGENC_H */
