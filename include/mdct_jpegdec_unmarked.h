/* mdct_jpegdec_unmarked.h -- C-ABI of libmdct_jpegdec_unmarked.so: baseline JPEG scans WITHOUT restart markers -> quantised int16
 * coefficient planes on the GPU.
 *
 * Most JPEG files carry no DRI segment: their scan is one interval, several MB long.  This library decodes such a scan into the same
 * coefficient planes mdct_jpegdec_decode (include/mdct_jpegdec.h) writes, with the same table handle (mdct_jpegdec_tables_create) and the
 * same descriptor (restart_interval must be 0).  The scan is cut into chunks of 8 KiB, one workgroup each; every chunk synchronises its
 * 256 sub-sequences as mdct_jpegdec_decode does inside an interval, and the chunks are synchronised with each other by a fixed number of
 * fix rounds, one launch each.  If the chunks' states had not converged after sync_rounds rounds, the status says so
 * (MDCT_JPEGDEC_NOT_SYNCHRONISED) and no level is written; sync_rounds >= the number of chunks, ceil(scan_len / 8192), always converges.
 *
 * Nothing is allocated or synchronised inside mdct_jpegdec_decode_unmarked, and its launch count depends only on the descriptor,
 * scan_len and sync_rounds: it may be captured into a hipGraph.  Return codes are those of include/mdct.h; the message of this library's
 * last failure is mdct_jpegdec_unmarked_last_error().  The library links against libmdct_jpegdec.so and libmdct_hip.so; its launches
 * appear in mdct_kernel_counts(). */
#ifndef MDCT_JPEGDEC_UNMARKED_H
#define MDCT_JPEGDEC_UNMARKED_H

#include "mdct_jpegdec.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MDCT_JPEGDEC_NOT_SYNCHRONISED 6 /* the chunks' states had not converged after sync_rounds fix rounds */

/* bytes of device workspace a decode of this scan needs; 0 (message set) for a descriptor this path refuses: restart_interval != 0,
 * an invalid descriptor, or scan_len >= 2^28 (host function, no device) */
size_t mdct_jpegdec_unmarked_workspace(const mdct_jpegdec_scan *desc, size_t scan_len);

/* Decode one scan without restart markers (desc->restart_interval must be 0) into the component planes.  scan: device pointer to the
 * entropy-coded bytes between the SOS header and the next marker (EOI), still stuffed.  Every block the descriptor names is zeroed and
 * its levels written; nothing outside those blocks and the workspace is written and nothing outside [scan, scan + scan_len) is read,
 * whatever the scan holds.  Any marker inside the scan, RSTm included, is MDCT_JPEGDEC_UNEXPECTED_MARKER.
 * workspace: device memory of at least mdct_jpegdec_unmarked_workspace() bytes, 16-byte aligned, scratch between calls; after a call its
 * first uint32 is the last fix round in which some chunk's state changed (0: none did).
 * status: 2 device uint32 -- [0] MDCT_JPEGDEC_*, [1] number of blocks (in decoding order) decoded before the first error (all of the
 * scan's blocks for OK / LEFTOVER / UNEXPECTED_MARKER after the last block, 0 for NOT_SYNCHRONISED).
 * After an error at block n = status[1] the planes hold: blocks 0 .. n - 1 their levels, exactly; block n the levels decoded before the
 * error (its DC only once the difference was complete) and zeros elsewhere; every block after n zero.  NOT_SYNCHRONISED leaves every
 * block zero.  The DC predictor wraps as in mdct_jpegdec_decode: the level stored is (int16_t)pred.
 * sync_rounds >= 0 (4 is usually plenty). */
int mdct_jpegdec_decode_unmarked(const mdct_jpegdec_scan *desc, const mdct_jpegdec_tables *tables, const uint8_t *scan, size_t scan_len,
                                 void *workspace, size_t workspace_bytes, uint32_t *status, int sync_rounds, void *stream);

/* message of this library's last failure */
const char *mdct_jpegdec_unmarked_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MDCT_JPEGDEC_UNMARKED_H */
