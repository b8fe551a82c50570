// jpeg_encode_opt.hip -- JPEG encoding with Huffman tables made for the image (include/mdct_jpegenc_opt.h; ITU-T T.81 K.2): the symbol
// statistics of the planes about to be coded, the optimal tables for them (host), and coders that take the caller's tables
// (DESIGN.md section 4.9.2).
//
// Built into its own library, libmdct_jpegenc_opt.so, linked against libmdct_hip.so (launch tally).  As in jpeg_encode_scan.hip the
// coefficients are the engine's own: the forward passes, the quantiser and the zig-zag compaction are aan_passes.h's and the multiplier
// tables come from own_tables.h; the bits are written by HuffSeqCoder16 (huffman_rows.h).
//
// One kernel template, k_opt<H, V, STATS>, on the chunk skeleton it shares with k_scan_rows (scan_chunks.h; layouts and scan order:
// scan_order.h): one workgroup per restart interval, the interval worked through in chunks, a chunk in a transform phase and a symbols
// phase separated by a barrier.  The kernel's body -- the LDS, the table / ring / histogram set-up, the symbols phase and the epilogue --
// is opt_symbols.h's, shared with k_coef (jpeg_coef.hip), whose levels come from a coefficient plane; here the source is ScanChunks
// (pixels).  The host checks it shares with jpeg_encode_scan.hip and jpeg_coef.hip are scan_host.h's.
// <H, V> is the luma sampling of an interleaved scan (<2, 2>, <2, 1>, <1, 1>; 3 / 2 / 3 waves) or <0, 0>: ONE plane, interval = one block
// row, 4 waves, chunks of 256 blocks, scan order = lane order.
// STATS = false: the symbols phase is HuffSeqCoder16 with the caller's tables.  Unless the host found the tables complete, a walk
//   before it counts the symbols that have no code (a table entry of 0: such a symbol is then written as its amplitude bits alone).
// STATS = true: the symbols phase counts instead of coding: a histogram of 2 x 272 dwords per wave in LDS, filled with LDS atomic adds --
//   EOB and the symbols 0x01, 0x02 and 0x11, which most lanes of a wave hit at once, by a ballot and a population count per class instead
//   of up to 64 serialised atomics -- and added to the caller's histogram once per workgroup with vector atomics.  Integer sums: the
//   result does not depend on the order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "aan_passes.h" // aan_fwd_h, aan_fwd_v, fwd_v_quant_levels, compact_levels16
#include "host_error.h"
#include "launch_tally.h"
#include "mdct_jpegenc_opt.h"
#include "scan_chunks.h"
#include "opt_symbols.h"
#include "scan_host.h"
#include "wg_sync.h"

#pragma clang fp contract(off)

namespace mdct
{
namespace jpegenc_opt
{

static_assert(opt_symbols::kClass == MDCT_JPEGENC_OPT_HIST_CLASS, "counts per class");

struct OptArgs
{
  const uint8_t *px[3];
  size_t pitch[3];
  uint8_t *out; // segments, seg_stride apart, indexed by the interval
  uint32_t *seg_bytes, *ff_counts;
  uint32_t *hist;    // STATS: [2][272]
  uint32_t *uncoded; // coder: symbols without a code
  size_t seg_stride;
  OwnTables tb[2]; // luma, chroma (one plane: its table in [0]); qf in the pair order of the column pass
  DctConsts consts;
  uint32_t mcus_x, my0;
  uint32_t cls0;     // one plane: its class (0 luminance, 1 chrominance) in the histogram
  uint32_t complete; // coder: every baseline symbol has a code in the tables in use, nothing to count
  float dc_shift;    // 64 * 128
  uint32_t dc[2][12];  // size << 16 | code per DC category, 0: no code; one plane: its tables in [0]
  uint32_t ac[2][256]; // size << 16 | code per RRRRSSSS
};
static_assert(sizeof(OptArgs) <= 4096, "kernel argument block");

using namespace scan_order;
using opt_symbols::kHist;

template <int H, int V, bool STATS>
__global__ __launch_bounds__((64 * kWaves<H, V>)) void k_opt(OptArgs a)
{
  opt_symbols::opt_kernel_body<ScanChunks<H, V, OptArgs>, H, V, STATS>(a);
}

} // namespace jpegenc_opt
} // namespace mdct

using namespace mdct::jpegenc_opt;

namespace
{

void common_args(OptArgs &a)
{
  a.consts = mdct::DctConsts();
  a.dc_shift = 64.0f * 128.0f;
}

template <bool STATS>
int launch(const OptArgs &a, int h, int v, unsigned n_intervals, hipStream_t s)
{
  const dim3 grid(n_intervals);
  if (h == 0)
    MDCT_LAUNCH((k_opt<0, 0, STATS>), grid, dim3(64 * kWaves<0, 0>), 0, s, a);
  else if (h == 1)
    MDCT_LAUNCH((k_opt<1, 1, STATS>), grid, dim3(64 * kWaves<1, 1>), 0, s, a);
  else if (v == 1)
    MDCT_LAUNCH((k_opt<2, 1, STATS>), grid, dim3(64 * kWaves<2, 1>), 0, s, a);
  else
    MDCT_LAUNCH((k_opt<2, 2, STATS>), grid, dim3(64 * kWaves<2, 2>), 0, s, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : fail(MDCT_NOT_SUPPORTED, "launch: %s", hipGetErrorString(e));
}

} // namespace

extern "C" {

const char *mdct_jpegenc_opt_last_error(void) { return g_err; }

size_t mdct_jpegenc_opt_seg_stride(size_t blocks) { return (209 * blocks + 8 + 3) & ~(size_t)3; }

int mdct_jpegenc_opt_table(const uint32_t *counts, int n_symbols, uint8_t bits16[16], uint8_t *vals, int *nvals)
{
  if (!counts || !bits16 || !vals || !nvals)
    return fail(MDCT_INVALID_PARAMETER, "null counts / bits16 / vals / nvals");
  if (!((n_symbols >= 12 && n_symbols <= 16) || n_symbols == 256))
    return fail(MDCT_INVALID_PARAMETER, "%d symbols (12..16 for a DC class, 256 for an AC class)", n_symbols);
  uint64_t freq[257];
  int codesize[257], others[257];
  bool any = false;
  for (int i = 0; i < 257; i++)
  {
    freq[i] = i < n_symbols ? counts[i] : 0;
    any = any || freq[i] != 0;
    codesize[i] = 0;
    others[i] = -1;
  }
  if (!any)
    return fail(MDCT_INVALID_PARAMETER, "all %d counts are zero", n_symbols);
  freq[256] = 1; // the reserved symbol: it takes the all-ones code
  for (;;)
  { // K.2, Figure K.1: merge the two least frequent trees; ties go to the larger symbol
    int c1 = -1, c2 = -1;
    uint64_t v = UINT64_MAX;
    for (int i = 0; i <= 256; i++)
      if (freq[i] && freq[i] <= v)
      {
        v = freq[i];
        c1 = i;
      }
    v = UINT64_MAX;
    for (int i = 0; i <= 256; i++)
      if (freq[i] && freq[i] <= v && i != c1)
      {
        v = freq[i];
        c2 = i;
      }
    if (c2 < 0)
      break;
    freq[c1] += freq[c2];
    freq[c2] = 0;
    for (codesize[c1]++; others[c1] >= 0;)
    {
      c1 = others[c1];
      codesize[c1]++;
    }
    others[c1] = c2;
    for (codesize[c2]++; others[c2] >= 0;)
    {
      c2 = others[c2];
      codesize[c2]++;
    }
  }
  int bits[258] = {0};
  int longest = 0;
  for (int i = 0; i <= 256; i++)
    if (codesize[i])
    {
      bits[codesize[i]]++;
      longest = codesize[i] > longest ? codesize[i] : longest;
    }
  int i = longest;
  for (; i > 16; i--) // Figure K.3
    while (bits[i] > 0)
    {
      int j = i - 2;
      while (bits[j] == 0)
        j--;
      bits[i] -= 2;
      bits[i - 1]++;
      bits[j + 1] += 2;
      bits[j]--;
    }
  while (bits[i] == 0)
    i--;
  bits[i]--; // the reserved symbol leaves
  int p = 0;
  for (int l = 1; l <= longest; l++) // Figure K.4: by code length before the adjustment, then by value
    for (int j = 0; j < 256; j++)
      if (codesize[j] == l)
        vals[p++] = (uint8_t)j;
  for (int l = 1; l <= 16; l++)
    bits16[l - 1] = (uint8_t)bits[l];
  *nvals = p;
  return MDCT_SUCCESS;
}

int mdct_jpegenc_opt_stats(const mdct_jpegenc_scan_plane *planes, int n_planes, const float *lut_luma, const float *lut_chroma, int interleaved,
                           uint32_t *hist, void *stream)
{
  if (!planes || !lut_luma || !hist)
    return fail(MDCT_INVALID_PARAMETER, "null planes / luma table / hist");
  if (n_planes != 1 && n_planes != 3)
    return fail(MDCT_INVALID_PARAMETER, "%d planes (1 or 3)", n_planes);
  if (n_planes == 3 && !lut_chroma)
    return fail(MDCT_INVALID_PARAMETER, "null chroma table");
  if (interleaved != 0 && interleaved != 1)
    return fail(MDCT_INVALID_PARAMETER, "interleaved %d (0 or 1)", interleaved);
  if ((uintptr_t)hist & 3)
    return fail(MDCT_INVALID_PARAMETER, "hist is not 4-byte aligned");
  const bool mcu_order = interleaved && n_planes == 3;
  int h = 0, v = 0;
  size_t mcus_x = 0, mcus_y = 0;
  if (mcu_order)
  {
    const int rc = check_mcu_planes(planes, &h, &v, &mcus_x, &mcus_y);
    if (rc)
      return rc;
  }
  else
    for (int c = 0; c < n_planes; c++)
    {
      const int rc = check_block_plane(planes[c].px, planes[c].pitch, planes[c].width, planes[c].height, c);
      if (rc)
        return rc;
    }
  OptArgs a;
  memset(&a, 0, sizeof(a));
  mdct::OwnTables tb[2];
  int rc = fill_lut(lut_luma, tb[0], "luma");
  if (!rc && n_planes == 3)
    rc = fill_lut(lut_chroma, tb[1], "chroma");
  if (rc)
    return rc;
  common_args(a);
  a.hist = hist;
  const hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(hist, 0, sizeof(uint32_t) * kHist, s);
  if (e != hipSuccess)
    return fail(MDCT_NOT_SUPPORTED, "memset: %s", hipGetErrorString(e));
  if (mcu_order)
  {
    a.tb[0] = tb[0];
    a.tb[1] = tb[1];
    for (int c = 0; c < 3; c++)
    {
      a.px[c] = planes[c].px;
      a.pitch[c] = planes[c].pitch;
    }
    a.mcus_x = (uint32_t)mcus_x;
    return launch<true>(a, h, v, (unsigned)mcus_y, s);
  }
  for (int c = 0; c < n_planes; c++)
  {
    a.tb[0] = tb[c ? 1 : 0];
    a.cls0 = c ? 1 : 0;
    a.px[0] = planes[c].px;
    a.pitch[0] = planes[c].pitch;
    a.mcus_x = (uint32_t)(planes[c].width / 8);
    rc = launch<true>(a, 0, 0, (unsigned)(planes[c].height / 8), s);
    if (rc)
      return rc;
  }
  return MDCT_SUCCESS;
}

int mdct_jpegenc_opt_rows(const uint8_t *px, size_t pitch, const float *lut, size_t sizeX, size_t sizeY, size_t by0, size_t by1,
                          const mdct_jpegenc_opt_spec *dc, const mdct_jpegenc_opt_spec *ac, uint8_t *out, size_t seg_stride, uint32_t *seg_bytes,
                          uint32_t *ff_counts, uint32_t *uncoded, void *stream)
{
  if (!lut || !out || !seg_bytes || !ff_counts || !uncoded)
    return fail(MDCT_INVALID_PARAMETER, "null table / out / seg_bytes / ff_counts / uncoded");
  int rc = check_block_plane(px, pitch, sizeX, sizeY, 0);
  if (rc)
    return rc;
  if (by0 >= by1 || by1 > sizeY / 8)
    return fail(MDCT_INVALID_PARAMETER, "block rows [%zu, %zu) of %zu", by0, by1, sizeY / 8);
  if ((rc = check_seg_stride(seg_stride, out, mdct_jpegenc_opt_seg_stride(sizeX / 8), 209, sizeX / 8, "row", "1665 bits per block")))
    return rc;
  if ((uintptr_t)uncoded & 3)
    return fail(MDCT_INVALID_PARAMETER, "uncoded is not 4-byte aligned");
  OptArgs a;
  memset(&a, 0, sizeof(a));
  bool complete = true;
  if ((rc = spec_codes(dc, false, "DC specification", a.dc[0], &complete)) || (rc = spec_codes(ac, true, "AC specification", a.ac[0], &complete)))
    return rc;
  if ((rc = fill_lut(lut, a.tb[0], "quantisation")))
    return rc;
  common_args(a);
  a.complete = complete;
  a.px[0] = px;
  a.pitch[0] = pitch;
  a.out = out;
  a.seg_bytes = seg_bytes;
  a.ff_counts = ff_counts;
  a.uncoded = uncoded;
  a.seg_stride = seg_stride;
  a.mcus_x = (uint32_t)(sizeX / 8);
  a.my0 = (uint32_t)by0;
  return launch<false>(a, 0, 0, (unsigned)(by1 - by0), (hipStream_t)stream);
}

int mdct_jpegenc_opt_scan_rows(const mdct_jpegenc_scan_plane *planes, int n_planes, const float *lut_luma, const float *lut_chroma,
                               const mdct_jpegenc_opt_spec specs[4], size_t my0, size_t my1, uint8_t *out, size_t seg_stride, uint32_t *seg_bytes,
                               uint32_t *ff_counts, uint32_t *uncoded, void *stream)
{
  if (!planes || !lut_luma || !lut_chroma || !specs || !out || !seg_bytes || !ff_counts || !uncoded)
    return fail(MDCT_INVALID_PARAMETER, "null planes / table / specs / out / seg_bytes / ff_counts / uncoded");
  if (n_planes != 3)
    return fail(MDCT_INVALID_PARAMETER, "%d planes (an interleaved scan takes Y, Cb, Cr)", n_planes);
  int h, v;
  size_t mcus_x, mcus_y;
  int rc = check_mcu_planes(planes, &h, &v, &mcus_x, &mcus_y);
  if (rc)
    return rc;
  if (my0 >= my1 || my1 > mcus_y)
    return fail(MDCT_INVALID_PARAMETER, "MCU rows [%zu, %zu) of %zu", my0, my1, mcus_y);
  const size_t blocks = mcus_x * (size_t)(h * v + 2);
  if ((rc = check_seg_stride(seg_stride, out, mdct_jpegenc_opt_seg_stride(blocks), 209, blocks, "MCU row", "1665 bits per block")))
    return rc;
  if ((uintptr_t)uncoded & 3)
    return fail(MDCT_INVALID_PARAMETER, "uncoded is not 4-byte aligned");
  OptArgs a;
  memset(&a, 0, sizeof(a));
  bool complete = true;
  static const char *const names[4] = {"DC luminance specification", "AC luminance specification", "DC chrominance specification", "AC chrominance specification"};
  for (int w = 0; w < 4; w++)
    if ((rc = spec_codes(&specs[w], w & 1, names[w], (w & 1) ? a.ac[w >> 1] : a.dc[w >> 1], &complete)))
      return rc;
  if ((rc = fill_lut(lut_luma, a.tb[0], "luma")) || (rc = fill_lut(lut_chroma, a.tb[1], "chroma")))
    return rc;
  common_args(a);
  a.complete = complete;
  for (int c = 0; c < 3; c++)
  {
    a.px[c] = planes[c].px;
    a.pitch[c] = planes[c].pitch;
  }
  a.out = out;
  a.seg_bytes = seg_bytes;
  a.ff_counts = ff_counts;
  a.uncoded = uncoded;
  a.seg_stride = seg_stride;
  a.mcus_x = (uint32_t)mcus_x;
  a.my0 = (uint32_t)my0;
  return launch<false>(a, h, v, (unsigned)(my1 - my0), (hipStream_t)stream);
}

} // extern "C"
