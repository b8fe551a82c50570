// jpeg_decode_batch.hip -- the restart-marked baseline scans of many JPEG files -> quantised int16 coefficient planes in four launches
// (include/mdct_jpegdec_batch.h).
//
// Built into its own library, libmdct_jpegdec_batch.so, linked against libmdct_hip.so; its launches go through MDCT_LAUNCH, so the
// launch tally of libmdct_hip.so (mdct_kernel_counts) counts them too.  The device code is jpegdec_common.h's: decode_interval (the
// body of k_decode) and rst_walk / rst_scan (the bodies of mdct_jpegdec_index's passes).  What this file adds is the layer that puts
// the intervals and chunks of many scans into one grid each:
//
//   k_batch_walk<false>  index, pass 1: one workgroup per index chunk of the batch; the chunk table names its scan, whose record holds the
//                        IndexArgs mdct_jpegdec_index would have built for that scan alone (its own byte range, chunk size, counts, offsets)
//   k_batch_scan         index, pass 2: one workgroup per scan
//   k_batch_walk<true>   index, pass 3: as pass 1
//   k_decode_batch       one workgroup per restart interval of the batch.  The workgroup finds its scan by binary search over the
//                        prefix of the scans' interval counts (uniform: scalar loads and scalar compares), and runs decode_interval
//                        on the scan's record with the interval's index within the scan.
// A scan's record is read from global memory where k_decode reads its kernel arguments; nothing else differs.  No workgroup waits
// for another, and every loop has a bound (the search: 32 trips).
//
// The host plans without a device: descriptor and table checks with the single-scan library's messages, interval counts, the chunk
// table, the prefixes, equal Huffman specifications stored once.  mdct_jpegdec_batch_bind resolves the device addresses into one image
// the caller uploads.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "jpegdec_common.h"
#include "launch_tally.h"
#include "mdct_jpegdec_batch.h"

namespace mdct
{
namespace jpegdec
{

// one scan of the batch as the kernels read it
struct BatchScan
{
  DecArgs dec;          // scan / off / status / tab point at this scan's own part of the batch's arrays
  IndexArgs idx;        // likewise; counts = the scan's part of the status array
  uint32_t first_chunk; // of the scan's chunks in the batch's chunk grid
};
static_assert(sizeof(BatchScan) % 8 == 0, "records lie back to back");

struct BatchArgs
{
  const BatchScan *scans;
  const uint32_t *first;      // [n_scans + 1]: first interval of every scan, then the total
  const uint32_t *chunk_scan; // [n_chunks]
  uint32_t n_scans;
};

__global__ void __launch_bounds__(kThreads) k_decode_batch(BatchArgs b)
{
  const uint32_t wg = blockIdx.x;
  uint32_t lo = 0, hi = b.n_scans; // first[lo] <= wg < first[hi]
  for (int it = 0; it < 32 && hi - lo > 1; it++)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (b.first[mid] <= wg)
      lo = mid;
    else
      hi = mid;
  }
  decode_interval(b.scans[lo].dec, wg - b.first[lo]);
}

template <bool WRITE>
__global__ void __launch_bounds__(kThreads) k_batch_walk(BatchArgs b)
{
  const BatchScan &s = b.scans[b.chunk_scan[blockIdx.x]];
  rst_walk<WRITE>(s.idx, blockIdx.x - s.first_chunk);
}

__global__ void __launch_bounds__(1024) k_batch_scan(BatchArgs b) { rst_scan(b.scans[blockIdx.x].idx); }

} // namespace jpegdec
} // namespace mdct

using namespace mdct::jpegdec;

// the host's plan: the records with addresses relative to the arrays they will point into, resolved by mdct_jpegdec_batch_bind
struct mdct_jpegdec_batch_plan
{
  std::vector<BatchScan> scans;
  std::vector<size_t> byte_offset;
  std::vector<uint32_t> first, first_chunk, chunk_scan, table_set; // first, first_chunk: n_scans + 1
  std::vector<DevTables> tables;
  size_t at_first, at_chunks, at_tables, image_bytes; // the image's parts after the records
  BatchArgs args;                                      // as bound
  bool bound;
};

namespace
{
size_t align16(size_t n) { return (n + 15) / 16 * 16; }

// the specification's bytes as a key: equal keys, equal tables
std::string spec_key(const mdct_jpegdec_batch_scan &s)
{
  std::string k;
  for (int t = 0; t < 4; t++)
  {
    k.push_back(s.bits16[t] ? 1 : 0);
    if (!s.bits16[t])
      continue;
    k.append((const char *)s.bits16[t], 16);
    k.push_back((char)(s.nvals[t] & 0xFF));
    k.push_back((char)(s.nvals[t] >> 8));
    k.append((const char *)s.vals[t], (size_t)s.nvals[t]);
  }
  return k;
}
} // namespace

extern "C" {

const char *mdct_jpegdec_batch_last_error(void) { return g_err; }

int mdct_jpegdec_batch_plan_create(mdct_jpegdec_batch_plan **plan, const mdct_jpegdec_batch_scan *scans, size_t n_scans, size_t total_bytes,
                                   size_t *bad_scan)
{
  if (bad_scan)
    *bad_scan = n_scans;
  if (!plan)
    return fail(MDCT_INVALID_PARAMETER, "null plan");
  *plan = nullptr;
  if (!scans || n_scans == 0 || n_scans >= (1ull << 31))
    return fail(MDCT_INVALID_PARAMETER, "null scans or %zu of them", n_scans);
  mdct_jpegdec_batch_plan *p = new mdct_jpegdec_batch_plan;
  p->bound = false;
  p->scans.resize(n_scans);
  p->byte_offset.resize(n_scans);
  p->table_set.resize(n_scans);
  p->first.assign(1, 0);
  p->first_chunk.assign(1, 0);
  std::map<std::string, uint32_t> sets;
  uint64_t intervals = 0, chunks = 0;
  int rc = MDCT_SUCCESS;
  for (size_t i = 0; i < n_scans && !rc; i++)
  {
    const mdct_jpegdec_batch_scan &s = scans[i];
    const mdct_jpegdec_scan *d = &s.desc;
    if (bad_scan)
      *bad_scan = i;
    // the checks of mdct_jpegdec_decode and mdct_jpegdec_tables_create, in their order and with their messages
    if ((rc = check_scan_head(d, true, "empty MCU grid or restart interval 0 (scans without restart markers are not supported)")) ||
        (rc = check_components(d)))
      break;
    if (s.byte_len > total_bytes || s.byte_offset > total_bytes - s.byte_len)
    {
      rc = fail(MDCT_INVALID_PARAMETER, "scan %zu: bytes %zu + %zu lie outside the buffer of %zu", i, s.byte_offset, s.byte_len, total_bytes);
      break;
    }
    mdct_jpegdec_tables t;
    t.dev = nullptr;
    t.device = 0;
    DevTables built;
    if ((rc = build_tables(s.bits16, s.vals, s.nvals, &built, t.present)))
      break;
    BatchScan &r = p->scans[i];
    memset(&r, 0, sizeof(r));
    if ((rc = fill_geometry(d, &t, r.dec)))
      break;
    const uint64_t n = (d->mcus_x * d->mcus_y + d->restart_interval - 1) / d->restart_interval;
    r.dec.scan_len = s.byte_len;
    r.dec.restart = (uint32_t)(d->restart_interval < r.dec.total_mcus ? d->restart_interval : r.dec.total_mcus);
    r.dec.n_intervals = (uint32_t)n;
    index_chunks(s.byte_len, n, r.idx);
    r.first_chunk = (uint32_t)chunks;
    p->byte_offset[i] = s.byte_offset;
    const auto ins = sets.emplace(spec_key(s), (uint32_t)p->tables.size());
    if (ins.second)
      p->tables.push_back(built);
    p->table_set[i] = ins.first->second;
    for (uint32_t c = 0; c < r.idx.nchunks; c++)
      p->chunk_scan.push_back((uint32_t)i);
    intervals += n;
    chunks += r.idx.nchunks;
    p->first.push_back((uint32_t)intervals);
    p->first_chunk.push_back((uint32_t)chunks);
    if (intervals >= (1ull << 31))
      rc = fail(MDCT_NOT_SUPPORTED, "more than 2^31 restart intervals in one batch");
  }
  if (rc)
  {
    delete p;
    return rc;
  }
  if (bad_scan)
    *bad_scan = n_scans;
  p->at_first = align16(n_scans * sizeof(BatchScan));
  p->at_chunks = align16(p->at_first + (n_scans + 1) * sizeof(uint32_t));
  p->at_tables = align16(p->at_chunks + p->chunk_scan.size() * sizeof(uint32_t));
  p->image_bytes = p->at_tables + p->tables.size() * sizeof(DevTables);
  *plan = p;
  return MDCT_SUCCESS;
}

int mdct_jpegdec_batch_plan_destroy(mdct_jpegdec_batch_plan *plan)
{
  delete plan;
  return MDCT_SUCCESS;
}

size_t mdct_jpegdec_batch_scans(const mdct_jpegdec_batch_plan *p) { return p ? p->scans.size() : 0; }
size_t mdct_jpegdec_batch_intervals(const mdct_jpegdec_batch_plan *p) { return p ? p->first.back() : 0; }
size_t mdct_jpegdec_batch_offsets(const mdct_jpegdec_batch_plan *p) { return p ? p->first.back() + p->scans.size() : 0; }
size_t mdct_jpegdec_batch_chunks(const mdct_jpegdec_batch_plan *p) { return p ? p->chunk_scan.size() : 0; }
size_t mdct_jpegdec_batch_table_sets(const mdct_jpegdec_batch_plan *p) { return p ? p->tables.size() : 0; }
size_t mdct_jpegdec_batch_image_bytes(const mdct_jpegdec_batch_plan *p) { return p ? p->image_bytes : 0; }

size_t mdct_jpegdec_batch_first_interval(const mdct_jpegdec_batch_plan *p, size_t scan)
{
  return p && scan < p->first.size() ? p->first[scan] : (size_t)-1;
}

size_t mdct_jpegdec_batch_first_chunk(const mdct_jpegdec_batch_plan *p, size_t scan)
{
  return p && scan < p->first_chunk.size() ? p->first_chunk[scan] : (size_t)-1;
}

size_t mdct_jpegdec_batch_chunk_bytes(const mdct_jpegdec_batch_plan *p, size_t scan)
{
  return p && scan < p->scans.size() ? (size_t)p->scans[scan].idx.chunk : (size_t)-1;
}

size_t mdct_jpegdec_batch_chunk_scan(const mdct_jpegdec_batch_plan *p, size_t chunk)
{
  return p && chunk < p->chunk_scan.size() ? p->chunk_scan[chunk] : (size_t)-1;
}

size_t mdct_jpegdec_batch_table_set(const mdct_jpegdec_batch_plan *p, size_t scan)
{
  return p && scan < p->table_set.size() ? p->table_set[scan] : (size_t)-1;
}

int mdct_jpegdec_batch_bind(mdct_jpegdec_batch_plan *p, void *host_image, const void *device_image, const uint8_t *bytes, uint64_t *offsets,
                            uint32_t *status)
{
  if (!p || !host_image || !device_image || !offsets || !status)
    return fail(MDCT_INVALID_PARAMETER, "null plan / image / offsets / status");
  if ((uintptr_t)device_image & 15)
    return fail(MDCT_INVALID_PARAMETER, "the device image must be 16-byte aligned");
  const size_t n = p->scans.size();
  const uint8_t *dev = (const uint8_t *)device_image;
  const DevTables *tab = (const DevTables *)(dev + p->at_tables);
  uint8_t *h = (uint8_t *)host_image;
  memset(h, 0, p->image_bytes);
  BatchScan *recs = (BatchScan *)h;
  for (size_t i = 0; i < n; i++)
  {
    BatchScan r = p->scans[i];
    if (!bytes && r.dec.scan_len)
      return fail(MDCT_INVALID_PARAMETER, "null byte buffer");
    r.dec.scan = r.idx.scan = bytes + p->byte_offset[i];
    r.dec.off = r.idx.off = offsets + p->first[i] + i;
    r.dec.status = r.idx.counts = status + p->first[i];
    r.dec.tab = tab + p->table_set[i];
    recs[i] = r;
  }
  memcpy(h + p->at_first, p->first.data(), p->first.size() * sizeof(uint32_t));
  if (!p->chunk_scan.empty())
    memcpy(h + p->at_chunks, p->chunk_scan.data(), p->chunk_scan.size() * sizeof(uint32_t));
  memcpy(h + p->at_tables, p->tables.data(), p->tables.size() * sizeof(DevTables));
  p->args.scans = (const BatchScan *)dev;
  p->args.first = (const uint32_t *)(dev + p->at_first);
  p->args.chunk_scan = (const uint32_t *)(dev + p->at_chunks);
  p->args.n_scans = (uint32_t)n;
  p->bound = true;
  return MDCT_SUCCESS;
}

int mdct_jpegdec_batch_index(const mdct_jpegdec_batch_plan *p, void *stream)
{
  if (!p || !p->bound)
    return fail(MDCT_INVALID_PARAMETER, "null plan, or one that mdct_jpegdec_batch_bind has not bound");
  hipStream_t s = (hipStream_t)stream;
  const uint32_t nchunks = (uint32_t)p->chunk_scan.size();
  if (nchunks)
    MDCT_LAUNCH(k_batch_walk<false>, dim3(nchunks), dim3(kThreads), 0, s, p->args);
  MDCT_LAUNCH(k_batch_scan, dim3(p->args.n_scans), dim3(1024), 0, s, p->args);
  if (nchunks)
    MDCT_LAUNCH(k_batch_walk<true>, dim3(nchunks), dim3(kThreads), 0, s, p->args);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : hip_fail(e, "index launch");
}

int mdct_jpegdec_batch_decode(const mdct_jpegdec_batch_plan *p, void *stream)
{
  if (!p || !p->bound)
    return fail(MDCT_INVALID_PARAMETER, "null plan, or one that mdct_jpegdec_batch_bind has not bound");
  MDCT_LAUNCH(k_decode_batch, dim3(p->first.back()), dim3(kThreads), 0, (hipStream_t)stream, p->args);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : hip_fail(e, "decode launch");
}

} // extern "C"
