/* mdct_jpegdec.h -- C-ABI of libmdct_jpegdec.so: restart-marked baseline JPEG scans -> quantised int16 coefficient planes on the GPU.
 *
 * The decoder half of the engine's entropy stage.  mdct_fwd_u8_jpeg_scan / mdct_jpeg_pack_rows (include/mdct.h) write a stuffed scan
 * with RSTm between restart intervals; this library reads such a scan (or any baseline scan with restart markers, ITU-T T.81 Annex F)
 * back into the coefficient planes mdct_fwd_u8_i16 writes and mdct_inv_i16_u8(_batch) reads: level (v, u) of block (by, bx) at
 * row by*8 + v, column bx*8 + u, de-zig-zagged, NOT dequantised.
 *
 * Every restart interval is decoded by one workgroup, split across its lanes by self-synchronising sub-sequence decoding.
 * Nothing is allocated or synchronised inside mdct_jpegdec_index / mdct_jpegdec_decode: both may be captured into a hipGraph.
 * Status codes are those of include/mdct.h (0 MDCT_SUCCESS, 1 MDCT_INVALID_PARAMETER, 2 MDCT_NOT_SUPPORTED); the message of this
 * library's last failure is mdct_jpegdec_last_error().  The library links against libmdct_hip.so; its launches appear in
 * mdct_kernel_counts().
 *
 * Scans without restart markers (restart_interval 0, refused here) are decoded by libmdct_jpegdec_unmarked.so
 * (include/mdct_jpegdec_unmarked.h), with the same table handle and descriptor.
 * The scans of a progressive file (spectral selection and successive approximation) are decoded by libmdct_jpegdec_prog.so
 * (include/mdct_jpegdec_prog.h), with the same table handle, descriptor and index.
 * The restart-marked scans of many files at once, in four launches for the whole batch: libmdct_jpegdec_batch.so
 * (include/mdct_jpegdec_batch.h), with the same descriptor, checks and per-interval decoder.
 * Out of scope: arithmetic / 12-bit / lossless JPEG.  Chroma upsampling and colour conversion: include/mdct_jpegcolor.h. */
#ifndef MDCT_JPEGDEC_H
#define MDCT_JPEGDEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* interval_status values written by mdct_jpegdec_decode (6 is MDCT_JPEGDEC_NOT_SYNCHRONISED of mdct_jpegdec_unmarked.h) */
enum
{
  MDCT_JPEGDEC_OK = 0,                /* exactly the interval's MCUs, then its own 1-bit padding up to the interval's end */
  MDCT_JPEGDEC_OUT_OF_DATA = 1,       /* the interval ended (or is missing) before its last MCU was complete */
  MDCT_JPEGDEC_BAD_CODE = 2,          /* a bit pattern that is no code of the Huffman table in use */
  MDCT_JPEGDEC_COEF_OVERFLOW = 3,     /* a run / ZRL that moves the coefficient index beyond 63 */
  MDCT_JPEGDEC_UNEXPECTED_MARKER = 4, /* a marker inside the interval's data, or the marker after it is not RST(k mod 8) */
  MDCT_JPEGDEC_LEFTOVER = 5,          /* data after the last MCU that is more than the interval's padding */
  MDCT_JPEGDEC_EOBRUN_OVERFLOW = 7    /* progressive scans (mdct_jpegdec_prog.h): an end-of-band run that reaches past the interval's last block */
};

#define MDCT_JPEGDEC_MAX_COMPONENTS 3
#define MDCT_JPEGDEC_MAX_BLOCKS_PER_MCU 10 /* T.81 B.2.3 */

/* Huffman tables of one scan: slots 0 and 1 DC, slots 2 and 3 AC.  bits16[i] (16 counts) and vals[i] (nvals[i] values) exactly as a
 * DHT segment carries them (and as mdct_huffman_spec returns them); bits16[i] == NULL leaves slot i empty.  The decoding structures of
 * T.81 C.2 / F.2.2.3 are built on the host and uploaded once (hipMalloc + hipMemcpy on the current device).  An invalid specification
 * (codes over-subscribed, sum of the counts != nvals, more than 256 values, a DC category above 11 or an AC size above 10) is refused with
 * MDCT_INVALID_PARAMETER. */
typedef struct mdct_jpegdec_tables mdct_jpegdec_tables;
int mdct_jpegdec_tables_create(mdct_jpegdec_tables **tables, const uint8_t *const bits16[4], const uint8_t *const vals[4], const int nvals[4]);
int mdct_jpegdec_tables_destroy(mdct_jpegdec_tables *tables);
/* the validation of mdct_jpegdec_tables_create alone (host function, no device) */
int mdct_jpegdec_tables_check(const uint8_t *const bits16[4], const uint8_t *const vals[4], const int nvals[4]);

/* Where the restart intervals are: scan = device pointer to the entropy-coded bytes between the SOS header and EOI, still stuffed and with
 * their RSTm markers.  On completion interval_offsets[0] = 0, interval_offsets[j + 1] = the offset just after the j-th RSTm marker
 * (j < n_intervals - 1) and interval_offsets[n_intervals] = scan_len; an interval whose marker is missing gets scan_len + 2 (no data, no
 * marker).  Interval k's data is [interval_offsets[k], interval_offsets[k + 1] - 2) and the last one's [.., scan_len), except that 0xFF
 * bytes directly before an RSTm are fill bytes (T.81 B.1.1.2) and mdct_jpegdec_decode leaves them out of the interval.  Surplus markers
 * stay inside the last interval (the decoder reports them).  Whether the markers run RST0..RST7 in order is checked by
 * mdct_jpegdec_decode.  interval_status (n_intervals device uint32) is scratch here; mdct_jpegdec_decode writes it.  Three launches. */
int mdct_jpegdec_index(const uint8_t *scan, size_t scan_len, size_t n_intervals, uint64_t *interval_offsets, uint32_t *interval_status,
                       void *stream);

typedef struct mdct_jpegdec_component
{
  int16_t *coef;             /* device plane, pitch in elements, 16-byte aligned rows */
  size_t pitch;
  size_t blocks_x, blocks_y; /* the plane's extent in blocks: mcus_x * h <= blocks_x, mcus_y * v <= blocks_y */
  int h, v;                  /* blocks of this component per MCU horizontally / vertically: 1 or 2 */
  int dc_slot, ac_slot;      /* 0..1, 2..3 */
} mdct_jpegdec_component;

typedef struct mdct_jpegdec_scan
{
  int n_components;        /* 1..3; a non-interleaved scan is one component with h = v = 1 over the component's own block grid */
  mdct_jpegdec_component comp[MDCT_JPEGDEC_MAX_COMPONENTS];
  size_t mcus_x, mcus_y;   /* the MCU grid (T.81 A.2) */
  size_t restart_interval; /* MCUs per restart interval (DRI), > 0 */
} mdct_jpegdec_scan;

/* number of restart intervals of the scan desc describes: ceil(mcus_x * mcus_y / restart_interval), 0 for an invalid descriptor
 * (host function) */
size_t mdct_jpegdec_intervals(const mdct_jpegdec_scan *desc);

/* Decode every restart interval of the scan into the component planes.  The blocks of interval k are zeroed and its levels written (DC
 * predictors reset per interval and component); nothing outside the blocks the descriptor names is written and nothing outside
 * [scan, scan + scan_len) is read, whatever the scan or the offsets hold.  interval_offsets: n_intervals + 1 device uint64 as
 * mdct_jpegdec_index leaves them, or the row_offsets of mdct_jpeg_pack_rows / mdct_fwd_*_jpeg_scan when the producer knows them.
 * interval_status: n_intervals device uint32, MDCT_JPEGDEC_* per interval: the first error in decoding order.  One launch, one workgroup
 * per interval.
 * An interval that fails leaves this in its blocks: those before the failing block hold their levels, exactly; the failing block holds
 * the levels decoded before the error (its DC only once the difference was complete) and zeros elsewhere; every block after it is zero.
 * An interval that is UNEXPECTED_MARKER / LEFTOVER after its last block has all its blocks.  Other intervals are not
 * touched by it.
 * The DC predictor is a 32-bit sum of the differences; the level stored is its low 16 bits, (int16_t)pred.  T.81 keeps a conforming
 * stream's DC within 11 bits, so a sum beyond int16 is no error class here: it wraps, and the interval's status stays what it was. */
int mdct_jpegdec_decode(const mdct_jpegdec_scan *desc, const mdct_jpegdec_tables *tables, const uint8_t *scan, size_t scan_len,
                        const uint64_t *interval_offsets, uint32_t *interval_status, void *stream);

/* message of this library's last failure */
const char *mdct_jpegdec_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MDCT_JPEGDEC_H */
