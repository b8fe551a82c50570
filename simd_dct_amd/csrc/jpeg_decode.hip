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

__global__ void __launch_bounds__(kThreads) k_decode(DecArgs a)
{
  __shared__ DevTables T;
  __shared__ uint32_t exit_state[kThreads];
  __shared__ uint32_t lcomp[16];
  __shared__ int wtot[kThreads / 64];
  __shared__ uint32_t first_err, fin_word, fail_unit;
  const int tid = threadIdx.x;
  const uint32_t k = blockIdx.x;
  load_tables(a, T, lcomp, tid);
  if (tid == 0)
  {
    first_err = kNone;
    fin_word = kNone;
  }
  // the interval's data, clamped into the scan whatever the offsets say
  const uint64_t len = a.scan_len;
  const bool last = k + 1 == a.n_intervals;
  uint64_t s = a.off[k];
  const uint64_t next = a.off[k + 1];
  uint64_t e = last ? next : (next >= 2 ? next - 2 : 0);
  s = s < len ? s : len;
  e = e < len ? e : len;
  e = e > s ? e : s;
  // T.81 B.1.1.2: 0xFF bytes directly before the interval's RSTm are fill bytes, not data (a data 0xFF is always followed by its
  // stuffed zero).  The last interval's end is the scan's, which the caller gives without them.
  if (!last && next <= len)
    for (uint64_t i = 0, n = e - s; i < n && a.scan[e - 1] == 0xFF; i++)
      e--;
  const uint64_t sb = (e - s + kThreads - 1) / kThreads;
  const SubLane q = sub_lane(s, e, sb < 8 ? 8 : sb, tid, true);
  const uint32_t mcu0 = k * a.restart;
  const uint32_t nmcu = (a.total_mcus - mcu0) < a.restart ? a.total_mcus - mcu0 : a.restart;
  const uint32_t units = nmcu * a.g.upm;
  wg_sync();

  // ---- synchronisation: lane 0 starts exact, the others from a guess, until no start changes
  Lane L;
  uint32_t my_start = 0;
  speculate(a, T, lcomp, q, my_start, L);
  settle(a, T, lcomp, q, 0u, my_start, L, exit_state);

  // ---- blocks before each lane's start, and the DC predictors there (an idle lane counts nothing)
  const uint32_t unit0 = (uint32_t)wg_excl_scan(L.blocks, wtot);
  int pred[3];
  for (int c = 0; c < 3; c++)
    pred[c] = wg_excl_scan(L.dc[c], wtot);

  // ---- zero the interval's blocks.  The stores are numbered in 32 bits, whose division costs a fraction of the 64-bit one: units * 8 +
  // kThreads stays below 2^32 for an interval of fewer than 2^29 - 32 blocks (64 GiB of coefficients), and this kernel has never
  // zeroed a longer one
  zero_units<uint32_t>(a.g, mcu0, 0, units, tid, kThreads);
  __threadfence_block();
  wg_sync();

  // ---- the decode proper
  uint32_t stop = 0;
  if (q.active)
    stop = write_pass(a, T, lcomp, q, my_start, unit0, units, mcu0, pred, &first_err, &fin_word);
  wg_sync();
  if (first_err != kNone)
  {
    // The lanes after the one that met the interval's first error started from states of the speculating passes, which carry on past
    // such an error: what they wrote lies in blocks after the failing one and means nothing.  Those blocks go back to zero; the
    // failing block keeps the levels decoded before the error (stop < units in the lane that reported it).
    if ((uint32_t)tid == first_err >> 8)
      fail_unit = stop;
    __threadfence();
    wg_sync();
    zero_units<uint32_t>(a.g, mcu0, fail_unit + 1, units - (fail_unit + 1), tid, kThreads);
  }
  if (tid == 0)
  {
    uint32_t st = first_err != kNone ? (first_err & 0xFF) : (fin_word != kNone ? fin_word : (uint32_t)MDCT_JPEGDEC_OUT_OF_DATA);
    if (st == MDCT_JPEGDEC_OK && !last)
    {
      // the marker after the interval must be RST(k mod 8)
      const bool ok = next >= 2 && next <= len && next - 2 >= s && a.scan[next - 2] == 0xFF && a.scan[next - 1] == 0xD0 + (k & 7);
      if (!ok)
        st = MDCT_JPEGDEC_UNEXPECTED_MARKER;
    }
    a.status[k] = st;
  }
}

// ------------------------------------------------------------------------------------------------------------------ the index
struct IndexArgs
{
  const uint8_t *scan;
  uint64_t len, chunk;   // chunk: bytes per workgroup, a multiple of kThreads
  uint32_t nchunks, n_intervals;
  uint32_t *counts;      // [nchunks]: markers per chunk, then their exclusive prefix
  uint64_t *off;
};

__device__ __forceinline__ bool rst_at(const uint8_t *scan, uint64_t len, uint64_t p)
{
  return scan[p] == 0xFF && p + 1 < len && (scan[p + 1] & 0xF8) == 0xD0;
}

template <bool WRITE>
__global__ void __launch_bounds__(kThreads) k_rst_walk(IndexArgs a)
{
  __shared__ int wtot[kThreads / 64];
  __shared__ uint32_t base;
  const uint64_t per = a.chunk / kThreads;
  const uint64_t p0 = (uint64_t)blockIdx.x * a.chunk + threadIdx.x * per;
  const uint64_t p1 = p0 + per < a.len ? p0 + per : a.len;
  int n = 0;
  for (uint64_t p = p0; p < p1; p++)
    n += rst_at(a.scan, a.len, p);
  if (!WRITE)
  {
    const int lane = threadIdx.x & 63;
    const int tot = wave_incl_scan(n, lane);
    if (lane == 63)
      wtot[threadIdx.x >> 6] = tot;
    wg_sync();
    if (threadIdx.x == 0)
      a.counts[blockIdx.x] = (uint32_t)(wtot[0] + wtot[1] + wtot[2] + wtot[3]);
    return;
  }
  if (threadIdx.x == 0)
    base = a.counts[blockIdx.x];
  const int before = wg_excl_scan(n, wtot);
  uint64_t j = (uint64_t)base + before; // ordinal of this lane's first marker
  for (uint64_t p = p0; p < p1; p++)
    if (rst_at(a.scan, a.len, p))
    {
      if (j + 1 < a.n_intervals)
        a.off[j + 1] = p + 2;
      j++;
    }
}

__global__ void __launch_bounds__(1024) k_rst_scan(IndexArgs a)
{
  __shared__ int wtot[16];
  const uint32_t total = wg1024_excl_prefix(a.counts, a.counts, a.nchunks, wtot);
  if (threadIdx.x == 0)
  {
    a.off[0] = 0;
    a.off[a.n_intervals] = a.len;
  }
  for (uint64_t j = (uint64_t)total + threadIdx.x; j + 1 < a.n_intervals; j += 1024)
    a.off[j + 1] = a.len + 2; // no marker: no data
}

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
  a.len = scan_len;
  uint64_t chunk = (scan_len + n_intervals - 1) / n_intervals;
  chunk = chunk < 4096 ? 4096 : chunk;
  a.chunk = (chunk + kThreads - 1) / kThreads * kThreads;
  a.nchunks = (uint32_t)((scan_len + a.chunk - 1) / a.chunk); // <= n_intervals: the counts fit in the status array
  a.n_intervals = (uint32_t)n_intervals;
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
