// jpeg_encode_opt.hip -- JPEG encoding with Huffman tables made for the image (include/mdct_jpegenc_opt.h; ITU-T T.81 K.2): the symbol
// statistics of the planes about to be coded, the optimal tables for them (host), and coders that take the caller's tables
// (DESIGN.md section 4.9.2).
//
// Built into its own library, libmdct_jpegenc_opt.so, linked against libmdct_hip.so (launch tally).  As in jpeg_encode_scan.hip the
// coefficients are the engine's own: the forward passes, the quantiser and the zig-zag compaction are compiled from mdct_kernels.hip's
// MDCT_AAN_FWD_ONLY region and the multiplier tables come from own_tables.h; the bits are written by HuffSeqCoder16 (huffman_rows.h).
//
// One kernel template, k_opt<H, V, STATS>, on the chunk skeleton it shares with k_scan_rows (scan_chunks.h; layouts and scan order:
// scan_order.h): one workgroup per restart interval, the interval worked through in chunks, a chunk in a transform phase and a symbols
// phase separated by a barrier.  This kernel's own are the LDS, the table / ring / histogram set-up, the symbols phase and the
// epilogue.  The host checks it shares with jpeg_encode_scan.hip are scan_host.h's.
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

#include "aan_fwd.h"
#define MDCT_AAN_FWD_ONLY
#include "mdct_kernels.hip" // only its MDCT_AAN_FWD_ONLY region: aan_fwd_h, aan_fwd_v, fwd_v_quant_levels, compact_levels16
#include "host_error.h"
#include "launch_tally.h"
#include "mdct_jpegenc_opt.h"
#include "scan_chunks.h"
#include "scan_host.h"
#include "wg_sync.h"

#pragma clang fp contract(off)

namespace mdct
{
namespace jpegenc_opt
{

constexpr uint32_t kRing = 1024;                        // words of bit stream held in LDS (as k_scan_rows)
constexpr uint32_t kClass = MDCT_JPEGENC_OPT_HIST_CLASS; // counts per class
constexpr uint32_t kHist = 2 * kClass;

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

// SSSS of a DC difference as huff_dc_token codes it
__device__ __forceinline__ uint32_t dc_category(int diff)
{
  diff = diff > 2047 ? 2047 : (diff < -2047 ? -2047 : diff);
  return diff ? 32u - (uint32_t)__builtin_clz((uint32_t)(diff < 0 ? -diff : diff)) : 0u;
}

// RRRRSSSS of a 16-bit entry run << 12 | level as huff_ac_token12 codes it (0xF0 for the ZRL entry)
__device__ __forceinline__ uint32_t ac_symbol12(uint32_t e)
{
  int l;
  asm("v_bfe_i32 %0, %1, 0, 12" : "=v"(l) : "v"(e));
  const int amp = l + (l >> 31);
  int lead;
  asm("v_ffbh_i32 %0, %1" : "=v"(lead) : "v"(amp));
  const int s = l ? 32 - lead : 0;
  return ((e >> 12) << 4) | (uint32_t)s;
}

template <int H, int V, bool STATS>
__global__ __launch_bounds__((64 * kWaves<H, V>)) void k_opt(OptArgs a)
{
  using Chunks = ScanChunks<H, V, OptArgs>;
  constexpr int WAVES = kWaves<H, V>;
  constexpr uint32_t kThreads = Chunks::kThreads, M = Chunks::M;
  __shared__ uint32_t ac[STATS ? 1 : 2][256], dc[STATS ? 1 : 2][12];
  __shared__ __attribute__((aligned(16))) uint16_t rec_all[kThreads * kRec16Row];
  __shared__ uint32_t meta[2][kThreads]; // by slot; [chunk parity] (ScanChunks)
  __shared__ uint32_t ring[STATS ? 1 : kRing];
  __shared__ uint32_t tot[2][WAVES];
  __shared__ uint32_t ff_total;
  __shared__ uint32_t hist[STATS ? WAVES : 1][STATS ? kHist : 1]; // one histogram per wave
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t my = a.my0 + blockIdx.x;
  HuffSeqCoder16<WAVES, kRing> coder;
  if constexpr (STATS)
  {
    for (uint32_t i = tid; i < WAVES * kHist; i += kThreads)
      (&hist[0][0])[i] = 0;
  }
  else
  {
    for (uint32_t i = tid; i < 512; i += kThreads)
      (&ac[0][0])[i] = (&a.ac[0][0])[i];
    if (tid < 24)
      (&dc[0][0])[tid] = (&a.dc[0][0])[tid];
    if (tid == 0)
      ff_total = 0;
    for (uint32_t w = tid; w < kRing; w += kThreads)
      ring[w] = 0;
    coder.ring = ring;
    coder.tot = tot;
    coder.out_w = reinterpret_cast<uint32_t *>(a.out + (size_t)my * a.seg_stride);
  }
  Chunks chunks(a);
  chunks.init(tid, lane, wave, my, rec_all, meta);

  // ---- the symbols phase's block of this thread
  const SeqBlock sb = seq_block<H, V>(tid);
  const uint16_t *crec = rec_all + sb.slot * kRec16Row;
  const bool cls = H == 0 ? a.cls0 != 0 : sb.chroma;                       // the block's class in the histogram
  const uint32_t *cac = ac[(!STATS && sb.chroma) ? 1 : 0], *cdc = dc[(!STATS && sb.chroma) ? 1 : 0];
  const unsigned long long cls_mask = __ballot(cls);                       // the wave's chroma lanes
  uint32_t *whist = hist[STATS ? wave : 0];
  uint32_t par = 0, uncoded = 0;
  wg_sync(); // tables and the cleared ring / histograms
  for (uint32_t m0 = 0, chunk = 0; m0 < a.mcus_x; m0 += M, chunk++)
  {
    chunks.transform(m0, chunk, par);
    wg_sync(); // every block of the chunk is in LDS
    const ChunkBlock b = chunks.block(sb, m0, par);
    const bool live = b.live, blk_eob = b.eob;
    const int blk_dc = b.dc, pred = b.pred, blk_n = live ? b.n : 0;
    if constexpr (STATS)
    {
      uint32_t *h = whist + (cls ? kClass : 0u);
      if (live)
        atomicAdd(&h[dc_category(blk_dc - pred)], 1u);
      // a symbol that many lanes hold at once: one add per class and wave
      auto add_ballot = [&](bool p, uint32_t sym) {
        const unsigned long long m = __ballot(p);
        const uint32_t nl = (uint32_t)__popcll(m & ~cls_mask), nc = (uint32_t)__popcll(m & cls_mask);
        if (lane == 0)
        {
          if (nl)
            atomicAdd(&whist[16 + sym], nl);
          if (nc)
            atomicAdd(&whist[kClass + 16 + sym], nc);
        }
      };
      add_ballot(live && blk_eob, 0x00u);
      for (int i = 0; __ballot(i < blk_n) != 0; i++)
      { // the lanes' i-th entries together
        const bool on = i < blk_n;
        const uint32_t sym = on ? ac_symbol12(crec[i]) : 0xFFFFu;
        add_ballot(sym == 0x01u, 0x01u);
        add_ballot(sym == 0x02u, 0x02u);
        add_ballot(sym == 0x11u, 0x11u);
        if (on && sym != 0x01u && sym != 0x02u && sym != 0x11u)
          atomicAdd(&h[16 + sym], 1u);
      }
      wg_sync(); // every row of the chunk has been walked: the next chunk's transform may write them (the coder's last barrier)
    }
    else
    {
      if (!a.complete && live)
      { // the symbols this block needs that the tables do not code
        uncoded += (cdc[dc_category(blk_dc - pred)] >> 16) == 0 ? 1u : 0u;
        for (int i = 0; i < blk_n; i++)
          uncoded += (cac[ac_symbol12(crec[i])] >> 16) == 0 ? 1u : 0u;
        if (blk_eob)
          uncoded += (cac[0x00] >> 16) == 0 ? 1u : 0u;
      }
      coder.chunk(crec, blk_n, live, blk_dc, pred, blk_eob, cac, cdc);
    }
    par ^= 1;
  }
  if constexpr (STATS)
  {
    wg_sync();
    for (uint32_t i = tid; i < kHist; i += kThreads)
    {
      uint32_t s = 0;
#pragma unroll
      for (int w = 0; w < WAVES; w++)
        s += hist[w][i];
      if (s)
        atomicAdd(&a.hist[i], s);
    }
  }
  else
  {
    if (coder.ff)
      atomicAdd(&ff_total, coder.ff);
    if (uncoded)
      atomicAdd(a.uncoded, uncoded);
    wg_sync();
    if (tid == 0)
    {
      uint32_t ff_last;
      a.seg_bytes[my] = coder.finish(&ff_last);
      a.ff_counts[my] = ff_total + ff_last;
    }
  }
}

} // namespace jpegenc_opt
} // namespace mdct

using namespace mdct::jpegenc_opt;

namespace
{

// a specification -> size << 16 | code per symbol (T.81 Annex C); checked as mdct_jpegdec_tables_check checks one, and no symbol twice.
// complete: every baseline symbol of the class has a code.
int spec_codes(const mdct_jpegenc_opt_spec *sp, bool is_ac, const char *name, uint32_t *tab, bool *complete)
{
  const int cap = is_ac ? 256 : 12;
  memset(tab, 0, sizeof(uint32_t) * (size_t)cap);
  if (!sp || !sp->bits16 || !sp->vals)
    return fail(MDCT_INVALID_PARAMETER, "%s: null specification / counts / values", name);
  if (sp->nvals < 1 || sp->nvals > 256)
    return fail(MDCT_INVALID_PARAMETER, "%s: %d values (1..256)", name, sp->nvals);
  int total = 0;
  for (int l = 0; l < 16; l++)
    total += sp->bits16[l];
  if (total != sp->nvals)
    return fail(MDCT_INVALID_PARAMETER, "%s: the 16 counts add up to %d codes, %d values given", name, total, sp->nvals);
  uint32_t code = 0;
  bool seen[256] = {false};
  for (uint32_t l = 1, p = 0; l <= 16; l++)
  {
    const uint32_t n = sp->bits16[l - 1];
    for (uint32_t i = 0; i < n; i++, p++)
    {
      const int v = sp->vals[p];
      if (is_ac ? (v & 15) > 10 : v > 11)
        return fail(MDCT_INVALID_PARAMETER, "%s: value 0x%02x is not a baseline %s symbol", name, v, is_ac ? "AC" : "DC");
      if (seen[v])
        return fail(MDCT_INVALID_PARAMETER, "%s: value 0x%02x is named twice", name, v);
      seen[v] = true;
    }
    code += n;
    if (code >= (1u << l)) // no code may be all 1-bits, as libjpeg requires
      return fail(MDCT_INVALID_PARAMETER, "%s: codes over-subscribed at length %u", name, l);
    code <<= 1;
  }
  annex_c_codes(sp->bits16, sp->vals, sp->nvals, cap, tab);
  bool all = true;
  if (is_ac)
  {
    all = tab[0x00] && tab[0xF0];
    for (int r = 0; r < 16; r++)
      for (int s = 1; s <= 10; s++)
        all = all && tab[r << 4 | s];
  }
  else
    for (int s = 0; s < 12; s++)
      all = all && tab[s];
  *complete = *complete && all;
  return MDCT_SUCCESS;
}

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
