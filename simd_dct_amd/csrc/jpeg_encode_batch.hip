// jpeg_encode_batch.hip -- a batch of 8-bit RGB images -> the interleaved baseline scans of their JPEG files in three launches
// (include/mdct_jpegenc_batch.h).
//
// Built into its own library, libmdct_jpegenc_batch.so, linked against libmdct_hip.so; its launches go through MDCT_LAUNCH, so the
// launch tally of libmdct_hip.so (mdct_kernel_counts) counts them too.  The device code is shared with the single-image libraries:
// rgb_ycc_tile (rgb_ycc.h, the body of k_rgb_ycc), ScanChunks (scan_chunks.h) and HuffSeqCoder16 (huffman_rows.h) in the loop of
// k_scan_rows, PackRow (pack_rows.h) as k_pack_write<true> uses it.  What this file adds is the layer that puts the tiles and MCU rows
// of many images into one grid each:
//
//   k_batch_rgb_ycc<Kind, Planar>  one workgroup per front tile of the batch.  The workgroup finds its image by binary search over the
//                                  prefix of the images' tile counts (uniform: scalar loads and scalar compares) and runs rgb_ycc_tile on
//                                  the image's record with the tile's place within the image.
//   k_batch_scan_rows<H, V>        one workgroup per MCU row of the batch; the image by the same search over the prefix of the row
//                                  counts; then the loop of k_scan_rows on that image's planes, into that image's segment range.  The
//                                  quantiser multipliers are one pair of tables per batch, read from the argument segment as ever.
//   k_batch_pack                   one workgroup per MCU row of the batch; the row table names its image, whether a marker follows it
//                                  and which; its place is the sum of the stuffed lengths of all batch rows before it.
// An image's record is read from global memory where the single-image kernels read their arguments; nothing else differs.  No
// workgroup waits for another, every loop has a bound (the search: 32 trips), and each kernel reads only what the launch before it
// wrote.
//
// The host plans without a device: the checks of mdct_jpegenc_from_rgb and mdct_jpegenc_scan_rows with their messages (rgb_ycc.h,
// scan_host.h), the prefixes, the row table.  mdct_jpegenc_batch_bind resolves the device addresses into one image the caller uploads.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "aan_passes.h" // aan_fwd_h, aan_fwd_v, fwd_v_quant_levels, compact_levels16
#include "host_error.h"
#include "launch_tally.h"
#include "mdct_jpegenc_batch.h"
#include "pack_rows.h"
#include "rgb_ycc.h"
#include "scan_chunks.h"
#include "scan_host.h"
#include "wg_sync.h"

#pragma clang fp contract(off)

namespace mdct
{
namespace jpegenc_batch
{

using jpegenc::EncArgs;

constexpr uint32_t kRing = 1024;      // words of bit stream held in LDS (as k_scan_rows)
constexpr uint32_t kRowLast = 8;      // row table, word 0: bit 3 = the last row of its image, bits 0..2 = m of its RSTm,
constexpr uint32_t kRowImageShift = 4; // ... bits 4.. = the image

// one image of the batch as the kernels read it
struct BatchImage
{
  EncArgs enc;         // the front kernel's record; p[k].px / p[k].pitch are the planes the scan coder reads
  uint8_t *seg;        // the image's segments, seg_stride apart, indexed by the MCU row within the image
  uint64_t seg_stride;
  uint32_t mcus_x, mcus_y;
  uint32_t first_row, first_tile; // of the image's MCU rows / front tiles in the batch's grids
  uint32_t tiles_x, pad;
};
static_assert(sizeof(BatchImage) % 8 == 0, "records lie back to back");

struct BatchArgs
{
  const BatchImage *img;
  const uint32_t *first_row;  // [n_images + 1]: first MCU row of every image, then the total
  const uint32_t *first_tile; // [n_images + 1]
  const uint2 *row_tab;       // [n_rows]: .x = image << 4 | last << 3 | m, .y = the image's seg_stride
  uint32_t n_images, n_rows;
};

struct BatchScanArgs
{
  BatchArgs b;
  uint32_t *seg_bytes, *ff_counts; // by the batch-wide row index
  OwnTables tb[2];                 // luma, chroma; qf in the pair order of the column pass
  DctConsts consts;
  float dc_shift;      // 64 * 128
  uint32_t dc[2][12];  // size << 16 | code per DC category: luma, chroma
  uint32_t ac[2][256]; // size << 16 | code per RRRRSSSS
};
static_assert(sizeof(BatchScanArgs) <= 4096, "kernel argument block");

struct BatchPackArgs
{
  BatchArgs b;
  const uint32_t *seg_bytes, *ff_counts;
  uint8_t *out;
  unsigned long long capacity;
  unsigned long long *row_off; // [n_rows + 1]
};

// the image whose range of the prefix holds `at`: first[i] <= at < first[i + 1] (uniform; every image has at least one entry)
__device__ __forceinline__ uint32_t image_of(const uint32_t *first, uint32_t n_images, uint32_t at)
{
  uint32_t lo = 0, hi = n_images;
  for (int it = 0; it < 32 && hi - lo > 1; it++)
  {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (first[mid] <= at)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

template <int Kind, bool Planar>
__global__ __launch_bounds__(jpegenc::kWG) void k_batch_rgb_ycc(BatchArgs b)
{
  __shared__ uint4 lds[jpegenc::kStageSlots<Kind, Planar>];
  const BatchImage &r = b.img[image_of(b.first_tile, b.n_images, blockIdx.x)];
  const EncArgs a = r.enc;
  const uint32_t tile = blockIdx.x - r.first_tile, tiles_x = r.tiles_x;
  const uint32_t by = tile / tiles_x;
  jpegenc::rgb_ycc_tile<Kind, Planar>(a, (int)(tile - by * tiles_x), (int)by, lds);
}

using namespace scan_order;

template <int H, int V>
__global__ __launch_bounds__((64 * kWaves<H, V>)) void k_batch_scan_rows(BatchScanArgs a)
{
  using Chunks = ScanChunks<H, V, BatchScanArgs, true>;
  constexpr int WAVES = kWaves<H, V>;
  constexpr uint32_t kThreads = Chunks::kThreads, M = Chunks::M;
  __shared__ uint32_t ac[2][256], dc[2][12];
  __shared__ __attribute__((aligned(16))) uint16_t rec_all[kThreads * kRec16Row];
  __shared__ uint32_t meta[2][kThreads]; // by slot; [chunk parity] (ScanChunks)
  __shared__ uint32_t ring[kRing];
  __shared__ uint32_t tot[2][WAVES];
  __shared__ uint32_t ff_total;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t row = blockIdx.x;
  const BatchImage &im = a.b.img[image_of(a.b.first_row, a.b.n_images, row)];
  const uint32_t my = row - im.first_row, mcus_x = im.mcus_x;
  uint32_t *const out_w = reinterpret_cast<uint32_t *>(im.seg + (size_t)my * im.seg_stride);
  const uint8_t *const px0 = im.enc.p[0].px, *const px1 = im.enc.p[1].px, *const px2 = im.enc.p[2].px;
  const size_t pitch0 = im.enc.p[0].pitch, pitch1 = im.enc.p[1].pitch, pitch2 = im.enc.p[2].pitch;
  for (uint32_t i = tid; i < 512; i += kThreads)
    (&ac[0][0])[i] = (&a.ac[0][0])[i];
  if (tid < 24)
    (&dc[0][0])[tid] = (&a.dc[0][0])[tid];
  if (tid == 0)
    ff_total = 0;
  for (uint32_t w = tid; w < kRing; w += kThreads)
    ring[w] = 0;
  HuffSeqCoder16<WAVES, kRing> coder;
  coder.ring = ring;
  coder.tot = tot;
  coder.out_w = out_w;
  Chunks chunks(a, mcus_x);
  chunks.init(tid, lane, wave, my, rec_all, meta, px0, px1, px2, pitch0, pitch1, pitch2);

  // ---- the coding phase's block of this thread
  const SeqBlock sb = seq_block<H, V>(tid);
  const uint16_t *crec = rec_all + sb.slot * kRec16Row;
  const uint32_t *cac = ac[sb.chroma ? 1 : 0], *cdc = dc[sb.chroma ? 1 : 0];
  uint32_t par = 0;
  wg_sync(); // tables and the cleared ring
  for (uint32_t m0 = 0, chunk = 0; m0 < mcus_x; m0 += M, chunk++)
  {
    chunks.transform(m0, chunk, par);
    wg_sync(); // every block of the chunk is in LDS
    const ChunkBlock b = chunks.block(sb, m0, par);
    coder.chunk(crec, b.n, b.live, b.dc, b.pred, b.eob, cac, cdc);
    par ^= 1;
  }
  if (coder.ff)
    atomicAdd(&ff_total, coder.ff);
  wg_sync();
  if (tid == 0)
  {
    uint32_t ff_last;
    a.seg_bytes[row] = coder.finish(&ff_last);
    a.ff_counts[row] = ff_total + ff_last;
  }
}

// stuffed length of batch row i in the output, restart marker included
__device__ __forceinline__ unsigned long long batch_row_len(const BatchPackArgs &a, uint32_t i)
{
  const uint2 t = a.b.row_tab[i];
  return (unsigned long long)min(a.seg_bytes[i], t.y) + a.ff_counts[i] + ((t.x & kRowLast) ? 0u : 2u);
}

// One workgroup per row; the copy itself is PackRow's (pack_rows.h), the place the own-base sum of k_pack_write<true> (stages.hip).
__global__ __launch_bounds__(256) void k_batch_pack(BatchPackArgs a)
{
  __shared__ uint32_t wave_tot[4];
  __shared__ unsigned long long wave_sum[4];
  __shared__ __attribute__((aligned(16))) uint32_t stage[kPackStageWords];
  const uint32_t r = blockIdx.x;
  const uint2 tab = a.b.row_tab[r];
  const BatchImage &im = a.b.img[tab.x >> kRowImageShift];
  const uint32_t nb = min(a.seg_bytes[r], tab.y); // a length beyond the stride is not a row
  const size_t seg_stride = im.seg_stride;
  PackRow<false> row;
  row.begin(im.seg + (size_t)(r - im.first_row) * seg_stride, seg_stride, nb); // on its way while the row's place is worked out
  unsigned long long s = 0;
  for (uint32_t i0 = threadIdx.x; i0 < r; i0 += 4 * 256)
  { // four rows per thread and step: independent loads in flight
    unsigned long long l[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
      l[k] = i0 + 256 * k < r ? batch_row_len(a, i0 + 256 * k) : 0ull;
    s += (l[0] + l[1]) + (l[2] + l[3]);
  }
  const unsigned long long base = wg_sum256(s, wave_sum);
  const unsigned long long end = base + batch_row_len(a, r);
  if (threadIdx.x == 0)
  {
    a.row_off[r] = base;
    if (r + 1 == a.b.n_rows)
      a.row_off[a.b.n_rows] = end;
  }
  if (end > a.capacity)
    return; // does not fit: the caller sees row_off[n_rows] > capacity
  row.finish(a.out + base, !(tab.x & kRowLast), tab.x & 7, stage, wave_tot);
}

} // namespace jpegenc_batch
} // namespace mdct

using namespace mdct::jpegenc_batch;
using mdct::jpegenc::k420;
using mdct::jpegenc::k422;
using mdct::jpegenc::k444;

// the host's plan; the tables' addresses inside the device image are resolved by mdct_jpegenc_batch_bind
struct mdct_jpegenc_batch_plan
{
  std::vector<BatchImage> images;
  std::vector<uint32_t> first_row, first_tile; // n_images + 1
  std::vector<uint2> row_tab;
  int kind;
  bool planar;
  size_t at_first_row, at_first_tile, at_row_tab, image_bytes; // the image's parts after the records
  BatchScanArgs scan;                                          // tables as planned; b, seg_bytes, ff_counts as bound
  bool bound;
};

namespace
{
size_t align16(size_t n) { return (n + 15) / 16 * 16; }

template <int Kind>
void launch_front(bool planar, uint32_t tiles, hipStream_t s, const BatchArgs &b)
{
  if (planar)
    MDCT_LAUNCH((k_batch_rgb_ycc<Kind, true>), dim3(tiles), dim3(mdct::jpegenc::kWG), 0, s, b);
  else
    MDCT_LAUNCH((k_batch_rgb_ycc<Kind, false>), dim3(tiles), dim3(mdct::jpegenc::kWG), 0, s, b);
}
} // namespace

extern "C" {

const char *mdct_jpegenc_batch_last_error(void) { return g_err; }

int mdct_jpegenc_batch_plan_create(mdct_jpegenc_batch_plan **plan, const mdct_jpegenc_batch_image *images, size_t n_images, int layout,
                                   const float *lut_luma, const float *lut_chroma, size_t *bad_image)
{
  if (bad_image)
    *bad_image = n_images;
  if (!plan)
    return fail(MDCT_INVALID_PARAMETER, "null plan");
  *plan = nullptr;
  if (!images || n_images == 0 || n_images > MDCT_JPEGENC_BATCH_MAX_ROWS)
    return fail(MDCT_INVALID_PARAMETER, "null images or %zu of them (1..%d)", n_images, MDCT_JPEGENC_BATCH_MAX_ROWS);
  if (!lut_luma || !lut_chroma)
    return fail(MDCT_INVALID_PARAMETER, "null planes / table / out / seg_bytes / ff_counts");
  mdct_jpegenc_batch_plan *p = new mdct_jpegenc_batch_plan;
  p->bound = false;
  p->kind = 0;
  p->planar = false;
  memset(&p->scan, 0, sizeof(p->scan));
  p->images.resize(n_images);
  p->first_row.assign(1, 0);
  p->first_tile.assign(1, 0);
  uint64_t rows = 0, tiles = 0;
  int rc = MDCT_SUCCESS;
  if ((rc = fill_lut(lut_luma, p->scan.tb[0], "luma")) || (rc = fill_lut(lut_chroma, p->scan.tb[1], "chroma")))
  {
    delete p;
    return rc;
  }
  for (size_t i = 0; i < n_images && !rc; i++)
  {
    const mdct_jpegenc_batch_image &im = images[i];
    if (bad_image)
      *bad_image = i;
    BatchImage &r = p->images[i];
    memset(&r, 0, sizeof(r));
    // the checks of mdct_jpegenc_from_rgb, then those of mdct_jpegenc_scan_rows, in their order and with their messages
    int kind;
    bool planar;
    if ((rc = check_rgb_image(im.in, im.in_pitch, im.in_plane_stride, im.width, im.height, MDCT_JPEGENC_RGB, layout, im.planes, 3, r.enc, &kind, &planar)))
      break;
    mdct_jpegenc_scan_plane sp[3];
    for (int c = 0; c < 3; c++)
      sp[c] = mdct_jpegenc_scan_plane{im.planes[c].px, im.planes[c].pitch, im.planes[c].width, im.planes[c].height, im.planes[c].h, im.planes[c].v};
    int h, v;
    size_t mcus_x, mcus_y;
    if ((rc = check_mcu_planes(sp, &h, &v, &mcus_x, &mcus_y)))
      break;
    if (i == 0)
    {
      p->kind = kind;
      p->planar = planar;
    }
    else if (kind != p->kind)
    {
      rc = fail(MDCT_INVALID_PARAMETER, "luma sampling factors %dx%d differ from those of image 0: one subsampling per batch", h, v);
      break;
    }
    if (!im.seg)
    {
      rc = fail(MDCT_INVALID_PARAMETER, "null planes / table / out / seg_bytes / ff_counts");
      break;
    }
    const int bpm = h * v + 2;
    const size_t need = 208 * mcus_x * (size_t)bpm + 8; // mdct_jpegenc_scan_seg_stride
    if ((rc = check_seg_stride(im.seg_stride, im.seg, need, 208, mcus_x * (size_t)bpm, "MCU row", "worst case of F.1.2")))
      break;
    if (im.seg_stride > 0xFFFFFFFFull)
    {
      rc = fail(MDCT_INVALID_PARAMETER, "seg_stride %zu: below 2^32", im.seg_stride);
      break;
    }
    r.seg = im.seg;
    r.seg_stride = im.seg_stride;
    r.mcus_x = (uint32_t)mcus_x;
    r.mcus_y = (uint32_t)mcus_y;
    r.first_row = (uint32_t)rows;
    r.first_tile = (uint32_t)tiles;
    r.tiles_x = (uint32_t)((r.enc.X + 64 * mdct::jpegenc::kRun - 1) / (64 * mdct::jpegenc::kRun));
    const uint32_t tiles_y = (uint32_t)((r.enc.G + mdct::jpegenc::kRows - 1) / mdct::jpegenc::kRows);
    for (uint32_t y = 0; y < r.mcus_y && rows + y < MDCT_JPEGENC_BATCH_MAX_ROWS; y++)
      p->row_tab.push_back(make_uint2((uint32_t)i << kRowImageShift | (y + 1 == r.mcus_y ? kRowLast : 0u) | (y & 7), (uint32_t)im.seg_stride));
    rows += r.mcus_y;
    tiles += (uint64_t)r.tiles_x * tiles_y;
    p->first_row.push_back((uint32_t)rows);
    p->first_tile.push_back((uint32_t)tiles);
    if (rows > MDCT_JPEGENC_BATCH_MAX_ROWS)
    {
      if (bad_image)
        *bad_image = n_images;
      rc = fail(MDCT_NOT_SUPPORTED, "more than %d MCU rows in one batch (image %zu brings them to %llu)", MDCT_JPEGENC_BATCH_MAX_ROWS, i, (unsigned long long)rows);
    }
  }
  const HuffCodes &hc = huff_codes();
  if (!rc && !hc.ok)
    rc = fail(MDCT_NOT_SUPPORTED, "mdct_huffman_spec failed");
  if (rc)
  {
    delete p;
    return rc;
  }
  if (bad_image)
    *bad_image = n_images;
  memcpy(p->scan.dc, hc.dc, sizeof(p->scan.dc));
  memcpy(p->scan.ac, hc.ac, sizeof(p->scan.ac));
  p->scan.consts = mdct::DctConsts();
  p->scan.dc_shift = 64.0f * 128.0f;
  p->at_first_row = align16(n_images * sizeof(BatchImage));
  p->at_first_tile = align16(p->at_first_row + (n_images + 1) * sizeof(uint32_t));
  p->at_row_tab = align16(p->at_first_tile + (n_images + 1) * sizeof(uint32_t));
  p->image_bytes = p->at_row_tab + p->row_tab.size() * sizeof(uint2);
  *plan = p;
  return MDCT_SUCCESS;
}

int mdct_jpegenc_batch_plan_destroy(mdct_jpegenc_batch_plan *plan)
{
  delete plan;
  return MDCT_SUCCESS;
}

size_t mdct_jpegenc_batch_images(const mdct_jpegenc_batch_plan *p) { return p ? p->images.size() : 0; }
size_t mdct_jpegenc_batch_rows(const mdct_jpegenc_batch_plan *p) { return p ? p->first_row.back() : 0; }
size_t mdct_jpegenc_batch_tiles(const mdct_jpegenc_batch_plan *p) { return p ? p->first_tile.back() : 0; }
size_t mdct_jpegenc_batch_image_bytes(const mdct_jpegenc_batch_plan *p) { return p ? p->image_bytes : 0; }

size_t mdct_jpegenc_batch_first_row(const mdct_jpegenc_batch_plan *p, size_t image)
{
  return p && image < p->first_row.size() ? p->first_row[image] : (size_t)-1;
}

size_t mdct_jpegenc_batch_first_tile(const mdct_jpegenc_batch_plan *p, size_t image)
{
  return p && image < p->first_tile.size() ? p->first_tile[image] : (size_t)-1;
}

size_t mdct_jpegenc_batch_row_image(const mdct_jpegenc_batch_plan *p, size_t row)
{
  return p && row < p->row_tab.size() ? p->row_tab[row].x >> kRowImageShift : (size_t)-1;
}

size_t mdct_jpegenc_batch_row_last(const mdct_jpegenc_batch_plan *p, size_t row)
{
  return p && row < p->row_tab.size() ? (p->row_tab[row].x & kRowLast) != 0 : (size_t)-1;
}

size_t mdct_jpegenc_batch_row_marker(const mdct_jpegenc_batch_plan *p, size_t row)
{
  return p && row < p->row_tab.size() ? p->row_tab[row].x & 7 : (size_t)-1;
}

int mdct_jpegenc_batch_bind(mdct_jpegenc_batch_plan *p, void *host_image, const void *device_image, uint32_t *seg_bytes, uint32_t *ff_counts)
{
  if (!p || !host_image || !device_image || !seg_bytes || !ff_counts)
    return fail(MDCT_INVALID_PARAMETER, "null plan / image / seg_bytes / ff_counts");
  if ((uintptr_t)device_image & 15)
    return fail(MDCT_INVALID_PARAMETER, "the device image must be 16-byte aligned");
  if (((uintptr_t)seg_bytes | (uintptr_t)ff_counts) & 3)
    return fail(MDCT_INVALID_PARAMETER, "seg_bytes and ff_counts must be 4-byte aligned");
  const size_t n = p->images.size();
  const uint8_t *dev = (const uint8_t *)device_image;
  uint8_t *h = (uint8_t *)host_image;
  memset(h, 0, p->image_bytes);
  memcpy(h, p->images.data(), n * sizeof(BatchImage));
  memcpy(h + p->at_first_row, p->first_row.data(), p->first_row.size() * sizeof(uint32_t));
  memcpy(h + p->at_first_tile, p->first_tile.data(), p->first_tile.size() * sizeof(uint32_t));
  memcpy(h + p->at_row_tab, p->row_tab.data(), p->row_tab.size() * sizeof(uint2));
  BatchArgs &b = p->scan.b;
  b.img = (const BatchImage *)dev;
  b.first_row = (const uint32_t *)(dev + p->at_first_row);
  b.first_tile = (const uint32_t *)(dev + p->at_first_tile);
  b.row_tab = (const uint2 *)(dev + p->at_row_tab);
  b.n_images = (uint32_t)n;
  b.n_rows = p->first_row.back();
  p->scan.seg_bytes = seg_bytes;
  p->scan.ff_counts = ff_counts;
  p->bound = true;
  return MDCT_SUCCESS;
}

int mdct_jpegenc_batch_planes(const mdct_jpegenc_batch_plan *p, void *stream)
{
  if (!p || !p->bound)
    return fail(MDCT_INVALID_PARAMETER, "null plan, or one that mdct_jpegenc_batch_bind has not bound");
  const hipStream_t s = (hipStream_t)stream;
  const uint32_t tiles = p->first_tile.back();
  switch (p->kind)
  {
  case k444: launch_front<k444>(p->planar, tiles, s, p->scan.b); break;
  case k422: launch_front<k422>(p->planar, tiles, s, p->scan.b); break;
  default: launch_front<k420>(p->planar, tiles, s, p->scan.b); break;
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : fail(MDCT_NOT_SUPPORTED, "launch: %s", hipGetErrorString(e));
}

int mdct_jpegenc_batch_scan(const mdct_jpegenc_batch_plan *p, void *stream)
{
  if (!p || !p->bound)
    return fail(MDCT_INVALID_PARAMETER, "null plan, or one that mdct_jpegenc_batch_bind has not bound");
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid(p->scan.b.n_rows);
  if (p->kind == k444)
    MDCT_LAUNCH((k_batch_scan_rows<1, 1>), grid, dim3(64 * kWaves<1, 1>), 0, s, p->scan);
  else if (p->kind == k422)
    MDCT_LAUNCH((k_batch_scan_rows<2, 1>), grid, dim3(64 * kWaves<2, 1>), 0, s, p->scan);
  else
    MDCT_LAUNCH((k_batch_scan_rows<2, 2>), grid, dim3(64 * kWaves<2, 2>), 0, s, p->scan);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : fail(MDCT_NOT_SUPPORTED, "launch: %s", hipGetErrorString(e));
}

int mdct_jpegenc_batch_pack(const mdct_jpegenc_batch_plan *p, uint8_t *out, size_t out_capacity, uint64_t *row_offsets, void *stream)
{
  if (!p || !p->bound)
    return fail(MDCT_INVALID_PARAMETER, "null plan, or one that mdct_jpegenc_batch_bind has not bound");
  if (!out || !row_offsets)
    return fail(MDCT_INVALID_PARAMETER, "null out / row_offsets");
  if ((uintptr_t)row_offsets & 7)
    return fail(MDCT_INVALID_PARAMETER, "row_offsets 8-byte aligned");
  BatchPackArgs a;
  a.b = p->scan.b;
  a.seg_bytes = p->scan.seg_bytes;
  a.ff_counts = p->scan.ff_counts;
  a.out = out;
  a.capacity = out_capacity;
  a.row_off = reinterpret_cast<unsigned long long *>(row_offsets);
  MDCT_LAUNCH(k_batch_pack, dim3(a.b.n_rows), dim3(256), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : fail(MDCT_NOT_SUPPORTED, "launch: %s", hipGetErrorString(e));
}

} // extern "C"
