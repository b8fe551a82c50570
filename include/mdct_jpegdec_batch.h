/* mdct_jpegdec_batch.h -- C-ABI of libmdct_jpegdec_batch.so: the restart-marked baseline scans of many JPEG files -> quantised int16
 * coefficient planes in four launches, whatever the number of files.
 *
 * include/mdct_jpegdec.h decodes one scan per call: a table upload, three index launches and one decode launch each.  This library
 * runs the same per-interval decoder (csrc/jpegdec_common.h: decode_interval, the body of k_decode) and the same three index passes
 * over all restart intervals of all scans at once.  The host plans the batch (mdct_jpegdec_batch_plan_create: no device needed),
 * writes one image of it for the device (mdct_jpegdec_batch_bind: scan records, the prefix of their interval counts, the chunk table,
 * the Huffman table sets; the caller uploads it with one copy), and two entry points launch:
 *   mdct_jpegdec_batch_index   three launches: every scan's interval offsets, exactly what mdct_jpegdec_index writes for that scan alone
 *   mdct_jpegdec_batch_decode  one launch, one workgroup per restart interval of the batch
 * Neither allocates or synchronises: both may be captured into a hipGraph.  Status codes are those of include/mdct.h; the message of
 * this library's last failure is mdct_jpegdec_batch_last_error().  The library links against libmdct_hip.so; its launches appear in
 * mdct_kernel_counts().
 *
 * Per scan the guarantees of mdct_jpegdec_decode hold: nothing outside the blocks the scan's descriptor names is written, nothing
 * outside the scan's own byte range [byte_offset, byte_offset + byte_len) of the buffer is read, whatever the bytes hold; a missing or
 * surplus marker in one scan moves no offset of another.  Scans without restart markers and progressive scans are not taken. */
#ifndef MDCT_JPEGDEC_BATCH_H
#define MDCT_JPEGDEC_BATCH_H

#include "mdct_jpegdec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One scan of the batch.  desc: as for mdct_jpegdec_decode (planes are device pointers; restart_interval > 0).  The scan's
 * entropy-coded bytes are [byte_offset, byte_offset + byte_len) of the batch's byte buffer.  bits16 / vals / nvals: the scan's Huffman
 * specification as for mdct_jpegdec_tables_create (host pointers, read by mdct_jpegdec_batch_plan_create only). */
typedef struct mdct_jpegdec_batch_scan
{
  mdct_jpegdec_scan desc;
  size_t byte_offset, byte_len;
  const uint8_t *bits16[4];
  const uint8_t *vals[4];
  int nvals[4];
} mdct_jpegdec_batch_scan;

typedef struct mdct_jpegdec_batch_plan mdct_jpegdec_batch_plan;

/* Plan the batch on the host (no device is touched): every descriptor is checked as mdct_jpegdec_decode checks it and every
 * specification as mdct_jpegdec_tables_create does, with the same messages; equal specifications share one table set.  total_bytes:
 * the size of the byte buffer, which every scan's range must lie in.  On a refusal *bad_scan (if not NULL) is the scan refused, or
 * n_scans when the refusal is about the batch as a whole.  The scans' intervals are numbered in the order given: scan i owns
 * intervals [first_interval(i), first_interval(i + 1)) of the batch-wide status array and entries
 * [first_interval(i) + i, first_interval(i + 1) + i + 1) of the batch-wide offsets array (n_i + 1 entries, relative to the scan's own
 * first byte). */
int mdct_jpegdec_batch_plan_create(mdct_jpegdec_batch_plan **plan, const mdct_jpegdec_batch_scan *scans, size_t n_scans, size_t total_bytes,
                                   size_t *bad_scan);
int mdct_jpegdec_batch_plan_destroy(mdct_jpegdec_batch_plan *plan);

/* What was planned (host functions; 0 for a NULL plan, (size_t)-1 for an index out of range) */
size_t mdct_jpegdec_batch_scans(const mdct_jpegdec_batch_plan *plan);
size_t mdct_jpegdec_batch_intervals(const mdct_jpegdec_batch_plan *plan);      /* of the whole batch: the status array's length */
size_t mdct_jpegdec_batch_offsets(const mdct_jpegdec_batch_plan *plan);        /* the offsets array's length: intervals + scans */
size_t mdct_jpegdec_batch_chunks(const mdct_jpegdec_batch_plan *plan);         /* index chunks of the whole batch */
size_t mdct_jpegdec_batch_table_sets(const mdct_jpegdec_batch_plan *plan);     /* distinct Huffman specifications */
size_t mdct_jpegdec_batch_first_interval(const mdct_jpegdec_batch_plan *plan, size_t scan); /* scan in 0..n_scans: the prefix */
size_t mdct_jpegdec_batch_first_chunk(const mdct_jpegdec_batch_plan *plan, size_t scan);    /* scan in 0..n_scans */
size_t mdct_jpegdec_batch_chunk_bytes(const mdct_jpegdec_batch_plan *plan, size_t scan);    /* the chunk size mdct_jpegdec_index cuts this scan by */
size_t mdct_jpegdec_batch_chunk_scan(const mdct_jpegdec_batch_plan *plan, size_t chunk);    /* the chunk table: whose chunk it is */
size_t mdct_jpegdec_batch_table_set(const mdct_jpegdec_batch_plan *plan, size_t scan);      /* the scan's table set */

/* The plan's device image.  mdct_jpegdec_batch_bind writes mdct_jpegdec_batch_image_bytes(plan) bytes to host_image (host memory of
 * the caller's), with every device address resolved: device_image is where the caller will put those bytes on the device (16-byte
 * aligned), bytes the device byte buffer, offsets (mdct_jpegdec_batch_offsets uint64) and status (mdct_jpegdec_batch_intervals uint32)
 * the device arrays the launches write.  Host function; the caller copies host_image to device_image before the first launch and may
 * bind again for other addresses. */
size_t mdct_jpegdec_batch_image_bytes(const mdct_jpegdec_batch_plan *plan);
int mdct_jpegdec_batch_bind(mdct_jpegdec_batch_plan *plan, void *host_image, const void *device_image, const uint8_t *bytes, uint64_t *offsets,
                            uint32_t *status);

/* Three launches: the interval offsets of every scan (status is scratch here, as in mdct_jpegdec_index). */
int mdct_jpegdec_batch_index(const mdct_jpegdec_batch_plan *plan, void *stream);
/* One launch: every restart interval of the batch, interval k of scan i by the workgroup first_interval(i) + k, exactly as
 * mdct_jpegdec_decode decodes it; its MDCT_JPEGDEC_* status goes to status[first_interval(i) + k]. */
int mdct_jpegdec_batch_decode(const mdct_jpegdec_batch_plan *plan, void *stream);

/* message of this library's last failure */
const char *mdct_jpegdec_batch_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MDCT_JPEGDEC_BATCH_H */
