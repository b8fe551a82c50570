// jpeg_coef.hip -- JPEG in the coefficient domain (include/mdct_jpegcoef.h): quantised coefficient planes, as a
// decode leaves them, -> Huffman segments with the caller's tables in either scan form, their symbol statistics, and the lossless
// flips, transposes and quarter turns.  No DCT and no quantiser run here: what goes in comes out, or is reported.
//
// Built into its own library, libmdct_jpegcoef.so, linked against libmdct_hip.so (launch tally) and libmdct_jpegenc_opt.so (segment
// stride).
//
// k_coef<H, V, STATS> is k_opt (jpeg_encode_opt.hip) with another source of levels: the kernel body -- LDS, set-up, symbols phase,
// epilogue -- is opt_symbols.h's, the lane-to-block layout and the read-out of a block scan_chunks.h's ChunkGrid; this file's own is
// CoefChunks, whose "transform" phase is a fetch: a lane loads its block's 8 rows as 8 loads of 16 bytes (a wave's loads of one row
// are 1 KiB of consecutive plane), widens them into the val[64] that compact_levels16 (aan_passes.h)
// reads, clamps AC levels to +-1023 and counts those it had to clamp, and requests the next chunk's rows before the barrier.
//
// k_coef_transform: one wave per tile of 8 x 8 blocks of dst.  The blocks of src that land in the tile are a tile of 8 x 8 blocks too
// (mirrored and / or transposed as a whole); the wave loads it into LDS row by row -- 8 lanes x 16 bytes = the 128 consecutive bytes of
// one row of the tile --, and writes the dst tile the same way, each lane gathering its 8 levels from LDS with the transposition and
// the signs applied.  Loads and stores are both runs of 128 bytes for every operation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "aan_passes.h" // of it, compact_levels16
#include "host_error.h"
#include "coef_host.h"
#include "launch_tally.h"
#include "mdct_jpegcoef.h"
#include "scan_chunks.h"
#include "opt_symbols.h"
#include "scan_host.h"
#include "wg_sync.h"

namespace mdct
{
namespace jpegcoef
{

struct CoefArgs
{
  const int16_t *coef[3];
  size_t pitch[3]; // elements
  uint8_t *out;    // segments, seg_stride apart, indexed by the interval
  uint32_t *seg_bytes, *ff_counts;
  uint32_t *hist;            // STATS: [2][272]
  uint32_t *uncoded;         // coder: symbols without a code
  uint32_t *unrepresentable; // levels and DC differences that had to be clamped
  size_t seg_stride;
  uint32_t mcus_x, my0;
  uint32_t cls0;       // one plane: its class (0 luminance, 1 chrominance) in the histogram
  uint32_t complete;   // coder: every baseline symbol has a code in the tables in use, nothing to count
  uint32_t dc[2][12];  // size << 16 | code per DC category, 0: no code; one plane: its tables in [0]
  uint32_t ac[2][256]; // size << 16 | code per RRRRSSSS
};
static_assert(sizeof(CoefArgs) <= 4096, "kernel argument block");

using namespace scan_order;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// The coefficient source of the chunk skeleton (scan_chunks.h).
template <int H, int V, class Args>
struct CoefChunks : ChunkGrid<H, V, Args>
{
  using Grid = ChunkGrid<H, V, Args>;
  using Grid::a;
  using Grid::bx0;
  using Grid::last_blk;
  using Grid::M;
  using Grid::step;
  static constexpr bool kCountsLoss = true;

  size_t pitch;
  const int16_t *src_row;
  uint4 rows[8];
  uint32_t lost = 0; // AC levels of this lane's blocks (inside the row) that had to be clamped

  __device__ __forceinline__ explicit CoefChunks(const Args &a_) : Grid(a_) {}

  // the 8 rows of block min(bx, last) of the block row (lanes past the row's end redo the last block); streamed once
  __device__ __forceinline__ void fetch(uint32_t bx)
  {
    const int16_t *src = src_row + (size_t)min(bx, last_blk) * 8;
#pragma unroll
    for (int r = 0; r < 8; r++)
    {
      const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(src + (size_t)r * pitch));
      rows[r] = make_uint4(v.x, v.y, v.z, v.w);
    }
  }

  __device__ __forceinline__ void init(uint32_t tid_, uint32_t lane, uint32_t wave, uint32_t my, uint16_t *rec_all, uint32_t (*meta_)[Grid::kThreads])
  {
    uint32_t comp, brow;
    bool chroma_wave;
    Grid::place(tid_, lane, wave, my, rec_all, meta_, comp, brow, chroma_wave);
    const size_t pitch0 = a.pitch[0], pitch1 = a.pitch[1], pitch2 = a.pitch[2];
    const int16_t *const c0 = a.coef[0], *const c1 = a.coef[1], *const c2 = a.coef[2];
    pitch = comp == 0 ? pitch0 : comp == 1 ? pitch1 : pitch2;
    src_row = (comp == 0 ? c0 : comp == 1 ? c1 : c2) + (size_t)brow * 8 * pitch;
    fetch(bx0);
  }

  // chunk number `chunk`, at MCU m0 of the row: rows -> levels (AC clamped to +-1023 and counted) -> entries in the lane's LDS row and
  // meta[par][tid]; then the next chunk's rows are requested.  The caller's barrier follows.
  __device__ __forceinline__ void transform(uint32_t m0, uint32_t chunk, uint32_t par)
  {
    uint32_t val[64];
    uint32_t clamped = 0;
#pragma unroll
    for (int r = 0; r < 8; r++)
    {
      const uint32_t w[4] = {rows[r].x, rows[r].y, rows[r].z, rows[r].w};
#pragma unroll
      for (int u = 0; u < 8; u++)
      {
        const int l = (u & 1) ? (int)w[u >> 1] >> 16 : (int)(int16_t)(w[u >> 1] & 0xFFFFu);
        if (r == 0 && u == 0)
          val[0] = (uint32_t)l & 0xFFFFu; // the DC level travels whole; its difference is judged in the symbols phase
        else
        {
          const int c = l > 1023 ? 1023 : (l < -1023 ? -1023 : l);
          clamped += c != l ? 1u : 0u;
          val[r * 8 + u] = (uint32_t)c & 0xFFFFu;
        }
      }
    }
    if (bx0 + chunk * step <= last_blk)
      lost += clamped;
    Grid::leave(val, par);
    if (m0 + M < a.mcus_x)
      fetch(bx0 + (chunk + 1) * step);
  }
};

template <int H, int V, bool STATS>
__global__ __launch_bounds__((64 * kWaves<H, V>)) void k_coef(CoefArgs a)
{
  opt_symbols::opt_kernel_body<CoefChunks<H, V, CoefArgs>, H, V, STATS>(a);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct XformArgs
{
  const int16_t *src;
  int16_t *dst;
  size_t spitch, dpitch;   // elements
  uint32_t sbx, sby;       // blocks of src
  uint32_t dbx, dby;       // blocks of dst
  uint32_t tiles_x, tiles; // tiles of 8 x 8 blocks of dst
  uint32_t transpose, flip_h, flip_v; // the operation: transpose, then mirror x, then mirror y
};

constexpr int kXformWaves = 4;
constexpr int kTileRow = 72; // halfwords per LDS row of a tile: 64 levels, padded, rows 16-byte aligned

__global__ __launch_bounds__(64 * kXformWaves) void k_coef_transform(XformArgs a)
{
  __shared__ __attribute__((aligned(16))) int16_t lds[kXformWaves][64 * kTileRow];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t tile = blockIdx.x * kXformWaves + wave;
  const bool on = tile < a.tiles;
  const uint32_t ty = on ? tile / a.tiles_x : 0, tx = on ? tile - ty * a.tiles_x : 0;
  // the dst tile, and the tile of the transposed-or-not intermediate that lands on it
  const uint32_t dy0 = ty * 8, dx0 = tx * 8;
  const uint32_t th = min(8u, a.dby - dy0), tw = min(8u, a.dbx - dx0);
  const uint32_t iy0 = a.flip_v ? a.dby - dy0 - th : dy0, ix0 = a.flip_h ? a.dbx - dx0 - tw : dx0;
  // ... which is this tile of src
  const uint32_t sy0 = a.transpose ? ix0 : iy0, sx0 = a.transpose ? iy0 : ix0;
  const uint32_t sth = a.transpose ? tw : th, stw = a.transpose ? th : tw;
  int16_t *tile_lds = lds[wave];
  const uint32_t seg = lane & 7, sub = lane >> 3;
  if (on && seg < stw)
  {
    const int16_t *src = a.src + (size_t)sy0 * 8 * a.spitch + (size_t)(sx0 + seg) * 8;
#pragma unroll
    for (uint32_t i = 0; i < 8; i++)
    {
      const uint32_t row = i * 8 + sub;
      if (row < sth * 8)
        *reinterpret_cast<uint4 *>(tile_lds + row * kTileRow + seg * 8) = *reinterpret_cast<const uint4 *>(src + (size_t)row * a.spitch);
    }
  }
  __syncthreads();
  if (on && seg < tw)
  {
    int16_t *dst = a.dst + (size_t)dy0 * 8 * a.dpitch + (size_t)(dx0 + seg) * 8;
    const uint32_t lx = a.flip_h ? tw - 1 - seg : seg; // the block column in the intermediate's tile
#pragma unroll
    for (uint32_t i = 0; i < 8; i++)
    {
      const uint32_t row = i * 8 + sub;
      if (row < th * 8)
      {
        const uint32_t y = row >> 3, v = row & 7;
        const uint32_t ly = a.flip_v ? th - 1 - y : y;
        const bool neg_v = a.flip_v && (v & 1);
        uint32_t w[4];
#pragma unroll
        for (uint32_t u = 0; u < 8; u++)
        {
          // intermediate [v][u] of block (ly, lx) = src [u][v] of block (lx, ly) when transposed
          const int16_t c = a.transpose ? tile_lds[(lx * 8 + u) * kTileRow + ly * 8 + v] : tile_lds[(ly * 8 + v) * kTileRow + lx * 8 + u];
          const bool neg = neg_v != (a.flip_h && (u & 1));
          const uint32_t x = (uint32_t)(neg ? -(int)c : (int)c) & 0xFFFFu;
          w[u >> 1] = (u & 1) ? (w[u >> 1] | x << 16) : x;
        }
        *reinterpret_cast<uint4 *>(dst + (size_t)row * a.dpitch) = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }
  }
}

} // namespace jpegcoef
} // namespace mdct

using namespace mdct::jpegcoef;
using mdct::opt_symbols::kHist;

namespace
{

static_assert(mdct::opt_symbols::kClass == MDCT_JPEGENC_OPT_HIST_CLASS, "counts per class");

template <bool STATS>
int launch(const CoefArgs &a, int h, int v, unsigned n_intervals, hipStream_t s)
{
  const dim3 grid(n_intervals);
  if (h == 0)
    MDCT_LAUNCH((k_coef<0, 0, STATS>), grid, dim3(64 * kWaves<0, 0>), 0, s, a);
  else if (h == 1)
    MDCT_LAUNCH((k_coef<1, 1, STATS>), grid, dim3(64 * kWaves<1, 1>), 0, s, a);
  else if (v == 1)
    MDCT_LAUNCH((k_coef<2, 1, STATS>), grid, dim3(64 * kWaves<2, 1>), 0, s, a);
  else
    MDCT_LAUNCH((k_coef<2, 2, STATS>), grid, dim3(64 * kWaves<2, 2>), 0, s, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : fail(MDCT_NOT_SUPPORTED, "launch: %s", hipGetErrorString(e));
}

// the byte range of the blocks a plane states
void plane_range(const mdct_jpegcoef_plane &p, uintptr_t *lo, uintptr_t *hi)
{
  *lo = (uintptr_t)p.coef;
  *hi = *lo + (((size_t)p.blocks_y * 8 - 1) * p.pitch + (size_t)p.blocks_x * 8) * sizeof(int16_t);
}

} // namespace

extern "C" {

const char *mdct_jpegcoef_last_error(void) { return g_err; }

int mdct_jpegcoef_stats(const mdct_jpegcoef_plane *planes, int n_planes, int interleaved, uint32_t *hist, uint32_t *unrepresentable, void *stream)
{
  if (!planes || !hist || !unrepresentable)
    return fail(MDCT_INVALID_PARAMETER, "null planes / hist / unrepresentable");
  if (n_planes != 1 && n_planes != 3)
    return fail(MDCT_INVALID_PARAMETER, "%d planes (1 or 3)", n_planes);
  if (interleaved != 0 && interleaved != 1)
    return fail(MDCT_INVALID_PARAMETER, "interleaved %d (0 or 1)", interleaved);
  int rc;
  if ((rc = check_word(hist, "hist")) || (rc = check_word(unrepresentable, "unrepresentable")))
    return rc;
  const bool mcu_order = interleaved && n_planes == 3;
  int h = 0, v = 0;
  uint32_t mcus_x = 0, mcus_y = 0;
  if (mcu_order)
  {
    if ((rc = check_coef_mcu_planes(planes, &h, &v, &mcus_x, &mcus_y)))
      return rc;
  }
  else
    for (int c = 0; c < n_planes; c++)
      if ((rc = check_coef_plane(planes[c], "plane", c)))
        return rc;
  CoefArgs a;
  memset(&a, 0, sizeof(a));
  a.hist = hist;
  a.unrepresentable = unrepresentable;
  const hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(hist, 0, sizeof(uint32_t) * kHist, s);
  if (e != hipSuccess)
    return fail(MDCT_NOT_SUPPORTED, "memset: %s", hipGetErrorString(e));
  if (mcu_order)
  {
    for (int c = 0; c < 3; c++)
    {
      a.coef[c] = planes[c].coef;
      a.pitch[c] = planes[c].pitch;
    }
    a.mcus_x = mcus_x;
    return launch<true>(a, h, v, mcus_y, s);
  }
  for (int c = 0; c < n_planes; c++)
  {
    a.cls0 = c ? 1 : 0;
    a.coef[0] = planes[c].coef;
    a.pitch[0] = planes[c].pitch;
    a.mcus_x = planes[c].blocks_x;
    if ((rc = launch<true>(a, 0, 0, planes[c].blocks_y, s)))
      return rc;
  }
  return MDCT_SUCCESS;
}

int mdct_jpegcoef_rows(const mdct_jpegcoef_plane *plane, size_t by0, size_t by1, const mdct_jpegenc_opt_spec *dc, const mdct_jpegenc_opt_spec *ac, uint8_t *out,
                       size_t seg_stride, uint32_t *seg_bytes, uint32_t *ff_counts, uint32_t *uncoded, uint32_t *unrepresentable, void *stream)
{
  if (!plane || !out || !seg_bytes || !ff_counts || !uncoded || !unrepresentable)
    return fail(MDCT_INVALID_PARAMETER, "null plane / out / seg_bytes / ff_counts / uncoded / unrepresentable");
  int rc = check_coef_plane(*plane, "plane", 0);
  if (rc)
    return rc;
  if (by0 >= by1 || by1 > plane->blocks_y)
    return fail(MDCT_INVALID_PARAMETER, "block rows [%zu, %zu) of %u", by0, by1, plane->blocks_y);
  if ((rc = check_seg_stride(seg_stride, out, mdct_jpegenc_opt_seg_stride(plane->blocks_x), 209, plane->blocks_x, "row", "1665 bits per block")))
    return rc;
  if ((rc = check_word(uncoded, "uncoded")) || (rc = check_word(unrepresentable, "unrepresentable")))
    return rc;
  CoefArgs a;
  memset(&a, 0, sizeof(a));
  bool complete = true;
  if ((rc = spec_codes(dc, false, "DC specification", a.dc[0], &complete)) || (rc = spec_codes(ac, true, "AC specification", a.ac[0], &complete)))
    return rc;
  a.complete = complete;
  a.coef[0] = plane->coef;
  a.pitch[0] = plane->pitch;
  a.out = out;
  a.seg_bytes = seg_bytes;
  a.ff_counts = ff_counts;
  a.uncoded = uncoded;
  a.unrepresentable = unrepresentable;
  a.seg_stride = seg_stride;
  a.mcus_x = plane->blocks_x;
  a.my0 = (uint32_t)by0;
  return launch<false>(a, 0, 0, (unsigned)(by1 - by0), (hipStream_t)stream);
}

int mdct_jpegcoef_scan_rows(const mdct_jpegcoef_plane *planes, int n_planes, const mdct_jpegenc_opt_spec specs[4], size_t my0, size_t my1, uint8_t *out,
                            size_t seg_stride, uint32_t *seg_bytes, uint32_t *ff_counts, uint32_t *uncoded, uint32_t *unrepresentable, void *stream)
{
  if (!planes || !specs || !out || !seg_bytes || !ff_counts || !uncoded || !unrepresentable)
    return fail(MDCT_INVALID_PARAMETER, "null planes / specs / out / seg_bytes / ff_counts / uncoded / unrepresentable");
  if (n_planes != 3)
    return fail(MDCT_INVALID_PARAMETER, "%d planes (an interleaved scan takes Y, Cb, Cr)", n_planes);
  int h, v;
  uint32_t mcus_x, mcus_y;
  int rc = check_coef_mcu_planes(planes, &h, &v, &mcus_x, &mcus_y);
  if (rc)
    return rc;
  if (my0 >= my1 || my1 > mcus_y)
    return fail(MDCT_INVALID_PARAMETER, "MCU rows [%zu, %zu) of %u", my0, my1, mcus_y);
  const size_t blocks = (size_t)mcus_x * (size_t)(h * v + 2);
  if ((rc = check_seg_stride(seg_stride, out, mdct_jpegenc_opt_seg_stride(blocks), 209, blocks, "MCU row", "1665 bits per block")))
    return rc;
  if ((rc = check_word(uncoded, "uncoded")) || (rc = check_word(unrepresentable, "unrepresentable")))
    return rc;
  CoefArgs a;
  memset(&a, 0, sizeof(a));
  bool complete = true;
  static const char *const names[4] = {"DC luminance specification", "AC luminance specification", "DC chrominance specification", "AC chrominance specification"};
  for (int w = 0; w < 4; w++)
    if ((rc = spec_codes(&specs[w], w & 1, names[w], (w & 1) ? a.ac[w >> 1] : a.dc[w >> 1], &complete)))
      return rc;
  a.complete = complete;
  for (int c = 0; c < 3; c++)
  {
    a.coef[c] = planes[c].coef;
    a.pitch[c] = planes[c].pitch;
  }
  a.out = out;
  a.seg_bytes = seg_bytes;
  a.ff_counts = ff_counts;
  a.uncoded = uncoded;
  a.unrepresentable = unrepresentable;
  a.seg_stride = seg_stride;
  a.mcus_x = mcus_x;
  a.my0 = (uint32_t)my0;
  return launch<false>(a, h, v, (unsigned)(my1 - my0), (hipStream_t)stream);
}

int mdct_jpegcoef_transform(const mdct_jpegcoef_plane *src, const mdct_jpegcoef_plane *dst, int op, void *stream)
{
  if (!src || !dst)
    return fail(MDCT_INVALID_PARAMETER, "null src / dst");
  if (op < MDCT_JPEGCOEF_FLIP_H || op > MDCT_JPEGCOEF_ROT270)
    return fail(MDCT_INVALID_PARAMETER, "operation %d (MDCT_JPEGCOEF_FLIP_H .. MDCT_JPEGCOEF_ROT270)", op);
  int rc;
  if ((rc = check_coef_plane(*src, "src", 0)) || (rc = check_coef_plane(*dst, "dst", 0)))
    return rc;
  // transpose, then mirror x, then mirror y (ROT270 = FLIP_H then TRANSPOSE = TRANSPOSE then FLIP_V)
  const bool t = op == MDCT_JPEGCOEF_TRANSPOSE || op == MDCT_JPEGCOEF_TRANSVERSE || op == MDCT_JPEGCOEF_ROT90 || op == MDCT_JPEGCOEF_ROT270;
  const bool fh = op == MDCT_JPEGCOEF_FLIP_H || op == MDCT_JPEGCOEF_ROT180 || op == MDCT_JPEGCOEF_ROT90 || op == MDCT_JPEGCOEF_TRANSVERSE;
  const bool fv = op == MDCT_JPEGCOEF_FLIP_V || op == MDCT_JPEGCOEF_ROT180 || op == MDCT_JPEGCOEF_ROT270 || op == MDCT_JPEGCOEF_TRANSVERSE;
  const uint32_t want_x = t ? src->blocks_y : src->blocks_x, want_y = t ? src->blocks_x : src->blocks_y;
  if (dst->blocks_x != want_x || dst->blocks_y != want_y)
    return fail(MDCT_INVALID_PARAMETER, "dst states %u x %u blocks; operation %d maps src's %u x %u to %u x %u", dst->blocks_x, dst->blocks_y, op, src->blocks_x,
                src->blocks_y, want_x, want_y);
  uintptr_t slo, shi, dlo, dhi;
  plane_range(*src, &slo, &shi);
  plane_range(*dst, &dlo, &dhi);
  if (slo < dhi && dlo < shi)
    return fail(MDCT_INVALID_PARAMETER, "src and dst overlap");
  XformArgs a;
  memset(&a, 0, sizeof(a));
  a.src = src->coef;
  a.dst = dst->coef;
  a.spitch = src->pitch;
  a.dpitch = dst->pitch;
  a.sbx = src->blocks_x;
  a.sby = src->blocks_y;
  a.dbx = dst->blocks_x;
  a.dby = dst->blocks_y;
  a.tiles_x = (a.dbx + 7) / 8;
  a.tiles = a.tiles_x * ((a.dby + 7) / 8);
  a.transpose = t;
  a.flip_h = fh;
  a.flip_v = fv;
  MDCT_LAUNCH(k_coef_transform, dim3((a.tiles + kXformWaves - 1) / kXformWaves), dim3(64 * kXformWaves), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : fail(MDCT_NOT_SUPPORTED, "launch: %s", hipGetErrorString(e));
}

} // extern "C"
