/* mdct_jpegdec_prog.h -- C-ABI of libmdct_jpegdec_prog.so: the scans of a progressive JPEG (SOF2; ITU-T T.81 Annex G: spectral
 * selection, and successive approximation through mdct_jpegdec_prog_decode_approx) -> quantised int16 coefficient planes on the GPU.
 *
 * The reader of what libmdct_jpegprog.so (include/mdct_jpegprog.h) writes (Ah = Al = 0, restart markers in every scan), and of the
 * files libjpeg's standard scan script gives (Pillow's progressive=True, jpegtran -progressive).  A progressive file codes every component's coefficients in
 * several scans: a DC-first scan (ss = se = 0; one component, or all of them interleaved) and AC-band scans (1 <= ss <= se <= 63, one
 * component each, G.1.1.1.1), whose blocks may end in an end-of-band run (EOBn: this block and run - 1 further ones have no more levels
 * in the band).  A run never crosses a restart interval (G.1.2.2), so every interval is still independent: one workgroup decodes it,
 * split across its lanes by self-synchronising sub-sequence decoding, as mdct_jpegdec_decode (include/mdct_jpegdec.h) decodes a
 * baseline interval.  Table handle, scan descriptor, interval index (mdct_jpegdec_index) and status codes are those of mdct_jpegdec.h.
 *
 * Nothing is allocated or synchronised inside mdct_jpegdec_prog_decode: it may be captured into a hipGraph.  Return codes are those of
 * include/mdct.h; the message of this library's last failure is mdct_jpegdec_prog_last_error().  The library links against
 * libmdct_jpegdec.so and libmdct_hip.so; its launches appear in mdct_kernel_counts().
 *
 * Successive approximation (G.1.2) codes a coefficient's bits in several scans: a first scan (Ah = 0) gives the levels divided by
 * 1 << Al, each refinement scan (Ah = Al + 1) one more bit.  Of the five kinds of scan, the two first kinds are decoded as described
 * above, for any Al.  A DC refinement scan is one raw bit per block: the lanes of the interval's workgroup share its bytes, each
 * finding its first block by a prefix sum of the data bytes before it.  An AC refinement scan is decoded SEQUENTIALLY inside a restart
 * interval, by one lane of a one-wave workgroup (the wave loads and stores the blocks): how many bits a symbol consumes depends on
 * which coefficients of the block earlier scans left non-zero, so the sub-sequence scheme does not apply.  Intervals run in parallel.
 *
 * A scan without restart markers is not a kind of its own here: restart_interval == 0 stays refused, and the caller hands such a scan
 * over as ONE interval (restart_interval = mcus_x * mcus_y, interval_offsets = {0, scan_len} written by the host, no
 * mdct_jpegdec_index).  That is correct and not fast: one workgroup decodes a whole first or DC refinement scan, one LANE a whole AC
 * refinement scan (DESIGN.md 4.13 has the measured times).
 * Out of scope, refused and never decoded wrongly: arithmetic coding, 12-bit samples. */
#ifndef MDCT_JPEGDEC_PROG_H
#define MDCT_JPEGDEC_PROG_H

#include "mdct_jpegdec.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What the band (ss, se) asks of the descriptor:
 *   ss == se == 0          a DC-first scan: 1..3 components, interleaved with the descriptor's sampling factors (at most 10 blocks per
 *                          MCU) or one component with h = v = 1 over its own block grid.  Only dc_slot is used (0..1, present in the
 *                          table handle); ac_slot is ignored.
 *   1 <= ss <= se <= 63    an AC-band scan: exactly one component with h = v = 1.  Only ac_slot is used (2..3, present); dc_slot is
 *                          ignored.
 * Any other band is MDCT_INVALID_PARAMETER.  Planes, pitch, alignment, the MCU grid, restart_interval > 0 and the limit of 2^31 blocks
 * are checked as mdct_jpegdec_decode checks them. */

/* number of restart intervals of the scan: ceil(mcus_x * mcus_y / restart_interval); 0 (message set) for anything refused (host
 * function, no device) */
size_t mdct_jpegdec_prog_intervals(const mdct_jpegdec_scan *desc, int ss, int se);

/* Decode every restart interval of one scan of the band (ss, se) into the component planes.  scan, scan_len, interval_offsets and
 * interval_status as for mdct_jpegdec_decode; the offsets come from mdct_jpegdec_index.  One launch, one workgroup per interval.
 *
 * What is written:
 *   a DC-first scan writes position (0, 0) of every block the interval covers (DC predictors reset per interval and component) and
 *   nothing else;
 *   an AC-band scan stores the non-zero levels it decodes at their positions inside zig-zag ss..se and nothing else: the caller
 *   provides planes that are zero in the band (there is no zeroing pass: three band scans of a plane do not each sweep it).
 * No position outside the band, no block outside the descriptor and no byte outside [scan, scan + scan_len) is touched, whatever the
 * scan or the offsets hold.
 *
 * interval_status: MDCT_JPEGDEC_* per interval, classified as for baseline scans (exactly the interval's blocks, then 1-bit padding,
 * then RST(k mod 8)); the first error in decoding order.  In an AC band, a level run or a ZRL that moves the index beyond se + 1 (a
 * ZRL may end exactly at se + 1, as a ZRL may end at 64 in a baseline scan) is COEF_OVERFLOW; an end-of-band run that names more
 * blocks than the interval has left is EOBRUN_OVERFLOW.
 * An interval that fails leaves this: the blocks before the failing one hold their levels, exactly; the failing block holds what was
 * decoded of it before the error (the block in which an overflowing EOBn was met is the failing one; the DC position of a failing
 * block of a DC scan is not written); in every later block of the interval the band's positions are 0 (position (0, 0) for a DC scan).
 * Other intervals are not touched by it.  The DC predictor wraps as in mdct_jpegdec_decode: the level stored is (int16_t)pred. */
int mdct_jpegdec_prog_decode(const mdct_jpegdec_scan *desc, int ss, int se, const mdct_jpegdec_tables *tables, const uint8_t *scan,
                             size_t scan_len, const uint64_t *interval_offsets, uint32_t *interval_status, void *stream);

/* The same for a scan with successive approximation (T.81 G.1.2): ah, al as the scan header gives them, 0 <= al <= 13 and ah == 0 (a
 * first scan) or ah == al + 1 (a refinement scan); anything else is MDCT_INVALID_PARAMETER, refused on the host before any launch, as
 * is everything mdct_jpegdec_prog_decode refuses.  mdct_jpegdec_prog_decode is the case ah = al = 0 of this function.  One launch.
 *
 *   DC first, al > 0       as above; the level stored is (int16_t)(pred << al).
 *   AC first, al > 0       as above; the level stored is v << al.  Statuses and the zeroing behind a failing block as above.
 *   DC refinement          one raw bit per block of the interval, in the scan's block order: a set bit ORs 1 << al into position
 *                          (0, 0).  No table is read: `tables` may be null, and dc_slot is only checked for its range.
 *   AC refinement          T.81 G.1.2.3, Figure G.7.  A symbol is (run, size) with size 0 or 1, or EOBn.  While `run` positions
 *                          without history are skipped, every position that is already non-zero consumes one correction bit; a set
 *                          bit adds +-(1 << al) away from zero where that bit of the coefficient is still clear; a new coefficient
 *                          is +-(1 << al).  The blocks of an end-of-band run consume the correction bits of their non-zero positions.
 *                          The component's ac_slot must be present.
 * interval_status of a refinement interval: as above (exactly the interval's blocks, then 1-bit padding, then RST(k mod 8)); in an AC
 * refinement a symbol of size > 1 is BAD_CODE, a run (a ZRL's sixteen positions included) that ends past se is COEF_OVERFLOW, an
 * EOBn that names more blocks than the interval has left is EOBRUN_OVERFLOW.  The first error in decoding order decides, and data
 * that runs out (or meets a marker) INSIDE a symbol comes before what that symbol would have said: an EOBn whose extra bits are cut
 * off is OUT_OF_DATA (UNEXPECTED_MARKER at a marker) whether or not the smallest run its code can name would still fit, and so is
 * a code, a sign bit or a correction bit the data ends in; sixteen bits that are no code are BAD_CODE only where sixteen bits of
 * data are left.  A lone 0xFF behind the data is a fill byte in front of RSTm and a marker (UNEXPECTED_MARKER) at the end of the
 * last interval.  A DC refinement interval is judged by its count of data bytes alone: fewer than its blocks' bits is OUT_OF_DATA
 * (UNEXPECTED_MARKER where a marker cut them short), a whole byte more or a 0-bit in the padding is LEFTOVER.
 * A refinement interval that fails touches nothing outside
 * the band and the interval's blocks; the blocks it reached hold unspecified refinements, and NOTHING is set back to zero (that
 * would destroy what earlier scans decoded): the caller discards the planes. */
int mdct_jpegdec_prog_decode_approx(const mdct_jpegdec_scan *desc, int ss, int se, int ah, int al,
                                    const mdct_jpegdec_tables *tables, const uint8_t *scan, size_t scan_len,
                                    const uint64_t *interval_offsets, uint32_t *interval_status, void *stream);

/* message of this library's last failure */
const char *mdct_jpegdec_prog_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* MDCT_JPEGDEC_PROG_H */
