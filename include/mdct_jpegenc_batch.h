/* mdct_jpegenc_batch.h -- C-ABI of libmdct_jpegenc_batch.so: a batch of 8-bit RGB images -> the interleaved baseline scans of their
 * JPEG files in three launches, whatever the number of images.
 *
 * include/mdct_jpegenc.h, include/mdct_jpegenc_scan.h and mdct_jpeg_pack_rows_counted (include/mdct.h) encode one image in three
 * launches.  This library runs the same three bodies over all images at once: the front tile of mdct_jpegenc_from_rgb
 * (csrc/rgb_ycc.h), the MCU-row coder of mdct_jpegenc_scan_rows (csrc/scan_chunks.h, HuffSeqCoder16) and the row packer of
 * mdct_jpeg_pack_rows_counted (csrc/pack_rows.h).  The host plans the batch (mdct_jpegenc_batch_plan_create: no device needed),
 * writes one image of the plan for the device (mdct_jpegenc_batch_bind: the images' records, the prefixes of their tile and MCU-row
 * counts, the packer's row table; the caller uploads it with one copy), and three entry points launch once each:
 *   mdct_jpegenc_batch_planes  every image -> its three padded planes on the MCU grid, exactly what mdct_jpegenc_from_rgb writes
 *   mdct_jpegenc_batch_scan    one workgroup per MCU row of the batch -> the row's segment in its image's segment range, its length
 *                              and 0xFF count at the batch-wide row index, exactly what mdct_jpegenc_scan_rows writes for that image
 *   mdct_jpegenc_batch_pack    one workgroup per MCU row of the batch -> every image's stuffed scan, RSTm between its rows, one after
 *                              the other in one buffer, each exactly what mdct_jpeg_pack_rows_counted writes for that image
 * None allocates or synchronises: all may be captured into a hipGraph.  One layout, one subsampling and one pair of quantisation
 * tables per batch.  Status codes are those of include/mdct.h; the message of this library's last failure is
 * mdct_jpegenc_batch_last_error().  The library links against libmdct_hip.so; its launches appear in mdct_kernel_counts(). */
#ifndef MDCT_JPEGENC_BATCH_H
#define MDCT_JPEGENC_BATCH_H

#include "mdct_jpegenc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the most MCU rows one batch may hold (every packing workgroup sums the lengths of the rows before its own) */
#define MDCT_JPEGENC_BATCH_MAX_ROWS 16384

/* One image of the batch.  in, in_pitch, in_plane_stride, width, height: the RGB input as for mdct_jpegenc_from_rgb (device pointer).
 * planes: Y, Cb, Cr as for mdct_jpegenc_from_rgb, PADDED TO THE MCU GRID as mdct_jpegenc_scan_rows takes them (width = mcus_x * 8 * h,
 * height = mcus_y * 8 * v).  seg: the image's own segment range (device pointer, 4-byte aligned): the segment of its MCU row r is at
 * seg + r * seg_stride; seg_stride a multiple of 4, at least mdct_jpegenc_scan_seg_stride(mcus_x, blocks per MCU) = 208 * mcus_x *
 * blocks per MCU + 8, below 2^32. */
typedef struct mdct_jpegenc_batch_image
{
  const uint8_t *in;
  size_t in_pitch, in_plane_stride;
  size_t width, height;
  mdct_jpegenc_plane planes[3];
  uint8_t *seg;
  size_t seg_stride;
} mdct_jpegenc_batch_image;

typedef struct mdct_jpegenc_batch_plan mdct_jpegenc_batch_plan;

/* Plan the batch on the host (no device is touched; the addresses are only compared).  layout: MDCT_JPEGENC_HWC or MDCT_JPEGENC_CHW,
 * for every image.  Every image is checked as mdct_jpegenc_from_rgb and mdct_jpegenc_scan_rows check it, with the same messages; all
 * must have the sampling factors of the first.  lut_luma / lut_chroma: HOST pointers to 64 floats, as for mdct_jpegenc_scan_rows.  On
 * a refusal *bad_image (if not NULL) is the image refused, or n_images when the refusal is about the batch as a whole (more than
 * MDCT_JPEGENC_BATCH_MAX_ROWS MCU rows among them).  The MCU rows are numbered in the order given: image i owns rows
 * [first_row(i), first_row(i + 1)) of the batch-wide seg_bytes, ff_counts and row_offsets arrays. */
int mdct_jpegenc_batch_plan_create(mdct_jpegenc_batch_plan **plan, const mdct_jpegenc_batch_image *images, size_t n_images, int layout,
                                   const float *lut_luma, const float *lut_chroma, size_t *bad_image);
int mdct_jpegenc_batch_plan_destroy(mdct_jpegenc_batch_plan *plan);

/* What was planned (host functions; 0 for a NULL plan, (size_t)-1 for an index out of range) */
size_t mdct_jpegenc_batch_images(const mdct_jpegenc_batch_plan *plan);
size_t mdct_jpegenc_batch_rows(const mdct_jpegenc_batch_plan *plan);                     /* MCU rows of the whole batch */
size_t mdct_jpegenc_batch_tiles(const mdct_jpegenc_batch_plan *plan);                    /* front tiles (1024 luma columns x 4 row groups) */
size_t mdct_jpegenc_batch_first_row(const mdct_jpegenc_batch_plan *plan, size_t image);  /* image in 0..n_images: the prefix */
size_t mdct_jpegenc_batch_first_tile(const mdct_jpegenc_batch_plan *plan, size_t image); /* image in 0..n_images */
size_t mdct_jpegenc_batch_row_image(const mdct_jpegenc_batch_plan *plan, size_t row);    /* the packer's row table: whose row it is, */
size_t mdct_jpegenc_batch_row_last(const mdct_jpegenc_batch_plan *plan, size_t row);     /* ... 1 if it is its image's last (no marker follows), */
size_t mdct_jpegenc_batch_row_marker(const mdct_jpegenc_batch_plan *plan, size_t row);   /* ... m of the RSTm after it: its index in its image & 7 */

/* The plan's device image.  mdct_jpegenc_batch_bind writes mdct_jpegenc_batch_image_bytes(plan) bytes to host_image (host memory of the
 * caller's), with every device address resolved: device_image is where the caller will put those bytes on the device (16-byte
 * aligned), seg_bytes and ff_counts the device arrays of mdct_jpegenc_batch_rows uint32 each that the scan launch writes and the
 * packing launch reads.  Host function; the caller copies host_image to device_image before the first launch and may bind again for
 * other addresses. */
size_t mdct_jpegenc_batch_image_bytes(const mdct_jpegenc_batch_plan *plan);
int mdct_jpegenc_batch_bind(mdct_jpegenc_batch_plan *plan, void *host_image, const void *device_image, uint32_t *seg_bytes, uint32_t *ff_counts);

/* One launch each, in this order on one stream. */
int mdct_jpegenc_batch_planes(const mdct_jpegenc_batch_plan *plan, void *stream);
int mdct_jpegenc_batch_scan(const mdct_jpegenc_batch_plan *plan, void *stream);
/* out: out_capacity bytes; row_offsets: mdct_jpegenc_batch_rows + 1 uint64 (8-byte aligned), all written: row r of the batch starts at
 * out + row_offsets[r], row_offsets[rows] is the total, and image i's scan is out[row_offsets[first_row(i)], row_offsets[first_row(i + 1)]).
 * A row that would end past out_capacity is not written: the caller sees row_offsets[rows] > out_capacity and may pack again into a
 * larger buffer (the segments are unchanged). */
int mdct_jpegenc_batch_pack(const mdct_jpegenc_batch_plan *plan, uint8_t *out, size_t out_capacity, uint64_t *row_offsets, void *stream);

/* message of this library's last failure */
const char *mdct_jpegenc_batch_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MDCT_JPEGENC_BATCH_H */
