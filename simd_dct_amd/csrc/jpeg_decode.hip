// jpeg_decode.hip -- restart-marked baseline JPEG scans -> quantised int16 coefficient planes (include/mdct_jpegdec.h).
//
// Built into its own library, libmdct_jpegdec.so, linked against libmdct_hip.so; its launches go through MDCT_LAUNCH, so the launch tally
// of libmdct_hip.so (mdct_kernel_counts) counts them too.
//
//   k_rst_walk<false>  index, pass 1: one workgroup per chunk of the scan counts the RSTm markers of its chunk (into the status scratch)
//   k_rst_scan         index, pass 2: one workgroup turns the chunk counts into exclusive prefixes, writes offsets 0 / n and the missing ones
//   k_rst_walk<true>   index, pass 3: every chunk writes the offset after each of its markers at the marker's ordinal
//   k_decode           one workgroup per restart interval.  The interval's stuffed bytes are cut into kThreads sub-sequences; lane i
//                      decodes from the start of its own with a guessed state and on past its end to the first symbol boundary, whose
//                      state (bit offset past the next sub-sequence's start, coefficient index, block within the MCU) it publishes.
//                      Lane i+1 decodes again from that state while it differs from the one it started from: the Huffman code
//                      re-synchronises within a few symbols, so the exit states stop changing after a few rounds (at most kThreads:
//                      lane 0's start is exact, and each round makes one more lane exact).  Block counts and per-component DC
//                      differences are then summed over the lanes (prefix sums), the interval's blocks zeroed, and every lane decodes
//                      its sub-sequence a last time, writing its levels (Weissenberger & Schmidt, ICPP 2018).
//                      While speculating, an invalid code (skip one bit) or a run past index 63 ends the block instead of stopping
//                      the lane: a lane that stopped would publish no usable state, and the lanes after it would become exact one
//                      round at a time.  From its exact start the last pass meets the same symbols; there such an error is the
//                      interval's status, and the blocks after the failing one are zeroed again (the lanes behind the error wrote
//                      levels of the re-synchronised decode into them).
// Byte unstuffing happens in the bit reader; positions a lane hands to the next are counted in bits after unstuffing from the next
// sub-sequence's first data byte, so both lanes count the same way.  Every loop has a bound; no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "jpegdec_common.h"
#include "launch_tally.h"

namespace mdct
{
namespace jpegdec
{

// the bodies are jpegdec_common.h's decode_interval / rst_walk / rst_scan, which libmdct_jpegdec_batch.so (jpeg_decode_batch.hip) runs
// over the intervals and chunks of many scans at once
__global__ void __launch_bounds__(kThreads) k_decode(DecArgs a) { decode_interval(a, blockIdx.x); }

template <bool WRITE>
__global__ void __launch_bounds__(kThreads) k_rst_walk(IndexArgs a)
{
  rst_walk<WRITE>(a, blockIdx.x);
}

__global__ void __launch_bounds__(1024) k_rst_scan(IndexArgs a) { rst_scan(a); }

} // namespace jpegdec
} // namespace mdct

using namespace mdct::jpegdec;

extern "C" {

const char *mdct_jpegdec_last_error(void) { return g_err; }

int mdct_jpegdec_tables_check(const uint8_t *const bits16[4], const uint8_t *const vals[4], const int nvals[4])
{
  bool present[4];
  return build_tables(bits16, vals, nvals, nullptr, present);
}

int mdct_jpegdec_tables_create(mdct_jpegdec_tables **tables, const uint8_t *const bits16[4], const uint8_t *const vals[4], const int nvals[4])
{
  if (!tables)
    return fail(MDCT_INVALID_PARAMETER, "null tables");
  *tables = nullptr;
  DevTables host;
  bool present[4];
  int rc = build_tables(bits16, vals, nvals, &host, present);
  if (rc)
    return rc;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess)
    return hip_fail(e, "hipGetDevice");
  DevTables *d = nullptr;
  if ((e = hipMalloc(&d, sizeof(DevTables))) != hipSuccess)
    return hip_fail(e, "hipMalloc");
  if ((e = hipMemcpy(d, &host, sizeof(DevTables), hipMemcpyHostToDevice)) != hipSuccess)
  {
    (void)hipFree(d);
    return hip_fail(e, "hipMemcpy");
  }
  mdct_jpegdec_tables *t = new mdct_jpegdec_tables;
  t->dev = d;
  t->device = dev;
  memcpy(t->present, present, sizeof(present));
  *tables = t;
  return MDCT_SUCCESS;
}

int mdct_jpegdec_tables_destroy(mdct_jpegdec_tables *tables)
{
  if (!tables)
    return MDCT_SUCCESS;
  const hipError_t e = hipFree(tables->dev);
  delete tables;
  return e == hipSuccess ? MDCT_SUCCESS : hip_fail(e, "hipFree");
}

static int check_desc(const mdct_jpegdec_scan *d, size_t *n_intervals)
{
  int rc = check_scan_head(d, true, "empty MCU grid or restart interval 0 (scans without restart markers are not supported)");
  if (rc || (rc = check_components(d)))
    return rc;
  *n_intervals = (d->mcus_x * d->mcus_y + d->restart_interval - 1) / d->restart_interval;
  return MDCT_SUCCESS;
}

size_t mdct_jpegdec_intervals(const mdct_jpegdec_scan *desc)
{
  size_t n = 0;
  return check_desc(desc, &n) ? 0 : n;
}

int mdct_jpegdec_index(const uint8_t *scan, size_t scan_len, size_t n_intervals, uint64_t *interval_offsets, uint32_t *interval_status, void *stream)
{
  if (!interval_offsets || !interval_status || (!scan && scan_len))
    return fail(MDCT_INVALID_PARAMETER, "null scan / offsets / status");
  if (n_intervals == 0 || n_intervals >= (1ull << 31))
    return fail(MDCT_INVALID_PARAMETER, "%zu intervals", n_intervals);
  IndexArgs a;
  a.scan = scan;
  index_chunks(scan_len, n_intervals, a); // nchunks <= n_intervals: the counts fit in the status array
  a.counts = interval_status;
  a.off = interval_offsets;
  hipStream_t s = (hipStream_t)stream;
  if (a.nchunks)
    MDCT_LAUNCH(k_rst_walk<false>, dim3(a.nchunks), dim3(kThreads), 0, s, a);
  MDCT_LAUNCH(k_rst_scan, dim3(1), dim3(1024), 0, s, a);
  if (a.nchunks)
    MDCT_LAUNCH(k_rst_walk<true>, dim3(a.nchunks), dim3(kThreads), 0, s, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : hip_fail(e, "index launch");
}

int mdct_jpegdec_decode(const mdct_jpegdec_scan *desc, const mdct_jpegdec_tables *tables, const uint8_t *scan, size_t scan_len,
                        const uint64_t *interval_offsets, uint32_t *interval_status, void *stream)
{
  size_t n = 0;
  int rc = check_desc(desc, &n);
  if (rc)
    return rc;
  if (!tables || !interval_offsets || !interval_status || (!scan && scan_len))
    return fail(MDCT_INVALID_PARAMETER, "null tables / scan / offsets / status");
  DecArgs a;
  memset(&a, 0, sizeof(a));
  a.scan = scan;
  a.scan_len = scan_len;
  a.off = interval_offsets;
  a.status = interval_status;
  if ((rc = fill_geometry(desc, tables, a)))
    return rc;
  a.restart = (uint32_t)(desc->restart_interval < a.total_mcus ? desc->restart_interval : a.total_mcus);
  a.n_intervals = (uint32_t)n;
  MDCT_LAUNCH(k_decode, dim3((uint32_t)n), dim3(kThreads), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : hip_fail(e, "decode launch");
}

} // extern "C"
