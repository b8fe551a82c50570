// jpeg_encode_scan.hip -- the three component planes of a colour JPEG encode -> the Huffman segments of ONE INTERLEAVED scan
// (include/mdct_jpegenc_scan.h; ITU-T T.81 A.2.3), one segment per MCU row.
//
// Built into its own library, libmdct_jpegenc_scan.so, linked against libmdct_hip.so (launch tally, Huffman specifications).  The
// coefficients are the engine's own: the forward passes, the quantiser and the zig-zag compaction are compiled from mdct_kernels.hip's
// own text (its MDCT_AAN_FWD_ONLY region, after aan_fwd.h) and the multiplier tables from own_tables.h -- the code k_px_huffman_rows
// and mdct_fwd_u8_i16 are built from, not a restatement.
//
// One kernel template, k_scan_rows<H, V> (luma sampling; chroma is 1x1): 4:2:0 <2, 2>, 4:2:2 <2, 1>, 4:4:4 <1, 1>.  One workgroup per
// MCU row; the row is worked through in chunks of kMcus MCUs = 64 * kWaves blocks, in two phases separated by a barrier:
//   transform  lane = block, COMPONENT-UNIFORM waves, so the quantiser multipliers stay wave-uniform scalar operands read from the
//              argument segment (two OwnTables, the wave picks one) and a wave's row loads are contiguous in one plane row:
//                4:2:0  wave 0 / 1: the upper / lower luma block row, blocks 2 m0 .. 2 m0 + 63; wave 2: Cb m0 .. m0 + 31 | Cr the same
//                4:2:2  wave 0: luma; wave 1: Cb | Cr                                                      (kMcus = 32)
//                4:4:4  wave 0 Y, wave 1 Cb, wave 2 Cr, blocks m0 .. m0 + 63                               (kMcus = 64)
//              Each lane leaves its block's entries in its LDS row and (DC, entry count, EOB flag) in meta[].
//   coding     thread s codes the s-th block of the chunk in scan order and reads the LDS row of the lane that transformed it; its
//              DC predictor is the previous block of the same component: a plain LDS read (meta[] of this chunk, or of the previous
//              chunk for the first block of a component -- meta is double-buffered --, or 0 at the row's start).
// The next chunk's pixel rows are loaded before the coding phase.  Lanes past the row's end redo the row's last block and are not live.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <mutex>

#include "aan_fwd.h"
#define MDCT_AAN_FWD_ONLY
#include "mdct_kernels.hip" // only its MDCT_AAN_FWD_ONLY region: aan_fwd_h, aan_fwd_v, fwd_v_quant_levels, compact_levels16
#include "huffman_rows.h"
#include "launch_tally.h"
#include "mdct_jpegenc_scan.h"
#include "own_tables.h"
#include "wg_sync.h"

#pragma clang fp contract(off)

namespace
{
char g_err[512];

int fail(int code, const char *fmt, ...)
{
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
} // namespace

namespace mdct
{
namespace jpegenc_scan
{

constexpr uint32_t kRing = 1024; // words of bit stream held in LDS (as k_px_huffman_rows; denser chunks take several windows)

struct ScanArgs
{
  const uint8_t *px[3];
  size_t pitch[3];
  uint8_t *out; // segments, seg_stride apart, indexed by the MCU row
  uint32_t *seg_bytes, *ff_counts;
  size_t seg_stride;
  OwnTables tb[2]; // luma, chroma; qf in the pair order of the column pass
  DctConsts consts;
  uint32_t mcus_x, my0;
  float dc_shift;      // 64 * 128
  uint32_t dc[2][12];  // size << 16 | code per DC category: luma, chroma
  uint32_t ac[2][256]; // size << 16 | code per RRRRSSSS
};
static_assert(sizeof(ScanArgs) <= 4096, "kernel argument block");

template <int H, int V> constexpr int kBlocksPerMcu = H * V + 2;
template <int H, int V> constexpr int kWaves = H == 2 ? V + 1 : 3;         // 4:2:0 3, 4:2:2 2, 4:4:4 3
template <int H, int V> constexpr uint32_t kMcus = H == 2 ? 32u : 64u;     // MCUs per chunk: 64 * kWaves blocks

// where the s-th block of a chunk in scan order was transformed (slot = wave * 64 + lane), where its predecessor of the same component
// was (pred; carry: it is the component's last block of the previous chunk), and whether it is a chroma block
struct SeqBlock
{
  uint32_t mcu, slot, pred;
  bool carry, chroma;
};

template <int H, int V>
__device__ __forceinline__ SeqBlock seq_block(uint32_t s)
{
  constexpr uint32_t B = kBlocksPerMcu<H, V>, M = kMcus<H, V>;
  const uint32_t i = s / B, k = s - i * B;
  SeqBlock b;
  b.mcu = i;
  if constexpr (H == 1)
  { // Y Cb Cr: wave k, lane i
    b.chroma = k > 0;
    b.slot = k * 64 + i;
    b.carry = i == 0;
    b.pred = b.carry ? k * 64 + 63 : b.slot - 1;
  }
  else
  {
    constexpr uint32_t NY = H * V, C0 = 64 * V; // luma blocks per MCU, the chroma wave's first slot
    b.chroma = k >= NY;
    if (k >= NY)
    { // Cb: lanes 0..31 of the chroma wave, Cr: lanes 32..63
      const uint32_t first = C0 + (k - NY) * M;
      b.slot = first + i;
      b.carry = i == 0;
      b.pred = b.carry ? first + M - 1 : b.slot - 1;
    }
    else if constexpr (V == 1)
    { // Y0 Y1: lanes 2i, 2i + 1 of wave 0
      b.slot = 2 * i + k;
      b.carry = b.slot == 0;
      b.pred = b.carry ? 63 : b.slot - 1;
    }
    else
    { // Y00 Y01 Y10 Y11: wave k >> 1 (the luma block row), lane 2i + (k & 1)
      b.slot = (k >> 1) * 64 + 2 * i + (k & 1);
      b.carry = s == 0;
      // Y00 follows the previous MCU's Y11, Y01 Y00, Y10 Y01, Y11 Y10
      b.pred = k == 0 ? (b.carry ? 127 : 64 + 2 * i - 1) : k == 1 ? 2 * i : k == 2 ? 2 * i + 1 : 64 + 2 * i;
    }
  }
  return b;
}

template <int H, int V>
__global__ __launch_bounds__((64 * kWaves<H, V>)) void k_scan_rows(ScanArgs a)
{
  constexpr int WAVES = kWaves<H, V>;
  constexpr uint32_t kThreads = 64 * WAVES, M = kMcus<H, V>;
  static_assert(kThreads == M * kBlocksPerMcu<H, V>, "one coding thread per block of the chunk");
  __shared__ uint32_t ac[2][256], dc[2][12];
  __shared__ __attribute__((aligned(16))) uint16_t rec_all[kThreads * kRec16Row];
  __shared__ uint32_t meta[2][kThreads]; // DC (low 16 bits) | entries << 16 | EOB needed << 24, by slot; [chunk parity]
  __shared__ uint32_t ring[kRing];
  __shared__ uint32_t tot[2][WAVES];
  __shared__ uint32_t ff_total;
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t my = a.my0 + blockIdx.x;
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
  coder.out_w = reinterpret_cast<uint32_t *>(a.out + (size_t)my * a.seg_stride);
  const DctConsts &C = a.consts;
  const AanPk &K = reinterpret_cast<const AanPk &>(C);

  // ---- the transform phase's block of this thread: plane, block row, first block and blocks per chunk
  const bool chroma_wave = H == 1 ? wave > 0 : wave == (uint32_t)V;
  uint32_t comp, bx0, step, last_blk, brow;
  if (H == 1)
  {
    comp = wave;
    bx0 = lane;
    step = 64;
    last_blk = a.mcus_x - 1;
    brow = my;
  }
  else if (!chroma_wave)
  {
    comp = 0;
    bx0 = lane;
    step = 64;
    last_blk = 2 * a.mcus_x - 1;
    brow = my * V + wave;
  }
  else
  {
    comp = 1 + (lane >> 5);
    bx0 = lane & 31;
    step = 32;
    last_blk = a.mcus_x - 1;
    brow = my;
  }
  // (selects, not an index: the argument block stays in scalar registers)
  const size_t pitch = comp == 0 ? a.pitch[0] : comp == 1 ? a.pitch[1] : a.pitch[2];
  const uint8_t *src_row = (comp == 0 ? a.px[0] : comp == 1 ? a.px[1] : a.px[2]) + (size_t)brow * 8 * pitch;
  uint2 rows[8];
  auto fetch = [&](uint32_t bx) { // the 8 rows of block min(bx, last) of the block row (lanes past the row's end redo the last block)
    const uint8_t *src = src_row + (size_t)min(bx, last_blk) * 8;
#pragma unroll
    for (int r = 0; r < 8; r++)
      rows[r] = load8(src + (size_t)r * pitch);
  };
  fetch(bx0);
  // the multiplier pairs of this wave's table (wave-uniform: scalar loads from the argument segment)
  const karg_pairs_t qf = karg_pairs(offsetof(ScanArgs, tb) + (chroma_wave ? sizeof(OwnTables) : 0) + offsetof(OwnTables, qf));
  uint16_t *rec = rec_all + tid * kRec16Row;

  // ---- the coding phase's block of this thread
  const SeqBlock sb = seq_block<H, V>(tid);
  const uint16_t *crec = rec_all + sb.slot * kRec16Row;
  const uint32_t *cac = ac[sb.chroma ? 1 : 0], *cdc = dc[sb.chroma ? 1 : 0];
  uint32_t par = 0;
  wg_sync(); // tables and the cleared ring
  for (uint32_t m0 = 0, chunk = 0; m0 < a.mcus_x; m0 += M, chunk++)
  {
    f32x2 P[4][8];
#pragma unroll
    for (int r = 0; r < 8; r++)
    {
      const f32x2 a01 = f32x2{ubyte_to_float<0>(rows[r].x), ubyte_to_float<1>(rows[r].x)};
      const f32x2 a23 = f32x2{ubyte_to_float<2>(rows[r].x), ubyte_to_float<3>(rows[r].x)};
      const f32x2 a45 = f32x2{ubyte_to_float<0>(rows[r].y), ubyte_to_float<1>(rows[r].y)};
      const f32x2 a67 = f32x2{ubyte_to_float<2>(rows[r].y), ubyte_to_float<3>(rows[r].y)};
      aan_fwd_h(K, a01, a23, a45, a67, P[0][r], P[1][r], P[2][r], P[3][r]);
    }
    uint32_t val[64];
    fwd_v_quant_levels<true>(K, P, qf, a.dc_shift, val);
    int my_dc;
    bool need_eob;
    const uint32_t n = compact_levels16(val, rec, my_dc, need_eob);
    meta[par][tid] = ((uint32_t)my_dc & 0xFFFFu) | n << 16 | (need_eob ? 1u << 24 : 0u);
    if (m0 + M < a.mcus_x)
      fetch(bx0 + (chunk + 1) * step); // in flight while this chunk is coded
    wg_sync(); // every block of the chunk is in LDS
    const uint32_t me = meta[par][sb.slot];
    const int pred = sb.carry ? (m0 == 0 ? 0 : (int)(int16_t)(meta[par ^ 1][sb.pred] & 0xFFFFu)) : (int)(int16_t)(meta[par][sb.pred] & 0xFFFFu);
    coder.chunk(crec, (int)((me >> 16) & 0xFFu), m0 + sb.mcu < a.mcus_x, (int)(int16_t)(me & 0xFFFFu), pred, (me >> 24) != 0, cac, cdc);
    par ^= 1;
  }
  if (coder.ff)
    atomicAdd(&ff_total, coder.ff);
  wg_sync();
  if (tid == 0)
  {
    uint32_t ff_last;
    a.seg_bytes[my] = coder.finish(&ff_last);
    a.ff_counts[my] = ff_total + ff_last;
  }
}

} // namespace jpegenc_scan
} // namespace mdct

using namespace mdct::jpegenc_scan;

namespace
{

// size << 16 | code of every symbol of the four Annex K tables (T.81 Annex C from mdct_huffman_spec), built once per process
struct HuffCodes
{
  uint32_t dc[2][12], ac[2][256];
  bool ok;
};

const HuffCodes &huff_codes()
{
  static HuffCodes t;
  static std::once_flag once;
  std::call_once(once, [] {
    memset(&t, 0, sizeof(t));
    t.ok = true;
    for (int which = 0; which < 4; which++)
    { // 0 DC luminance, 1 AC luminance, 2 DC chrominance, 3 AC chrominance
      uint8_t bits[16], vals[256];
      int nvals = 0;
      if (mdct_huffman_spec(which, bits, vals, &nvals) != MDCT_SUCCESS)
      {
        t.ok = false;
        return;
      }
      uint32_t *tab = (which & 1) ? t.ac[which >> 1] : t.dc[which >> 1];
      const int cap = (which & 1) ? 256 : 12;
      uint32_t code = 0;
      int k = 0;
      for (uint32_t len = 1; len <= 16; len++, code <<= 1)
        for (int i = 0; i < bits[len - 1] && k < nvals; i++, k++, code++)
          if (vals[k] < cap)
            tab[vals[k]] = len << 16 | code;
    }
  });
  return t;
}

} // namespace

extern "C" {

const char *mdct_jpegenc_scan_last_error(void) { return g_err; }

size_t mdct_jpegenc_scan_seg_stride(size_t mcus_x, int blocks_per_mcu) { return 208 * mcus_x * (size_t)(blocks_per_mcu > 0 ? blocks_per_mcu : 0) + 8; }

int mdct_jpegenc_scan_rows(const mdct_jpegenc_scan_plane *planes, int n_planes, const float *lut_luma, const float *lut_chroma, size_t my0,
                           size_t my1, uint8_t *out, size_t seg_stride, uint32_t *seg_bytes, uint32_t *ff_counts, void *stream)
{
  if (!planes || !lut_luma || !lut_chroma || !out || !seg_bytes || !ff_counts)
    return fail(MDCT_INVALID_PARAMETER, "null planes / table / out / seg_bytes / ff_counts");
  if (n_planes != 3)
    return fail(MDCT_INVALID_PARAMETER, "%d planes (an interleaved scan takes Y, Cb, Cr)", n_planes);
  for (int c = 0; c < 3; c++)
    if (!planes[c].px)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: null pointer", c);
  const int h = planes[0].h, v = planes[0].v;
  if (planes[1].h != 1 || planes[1].v != 1 || planes[2].h != 1 || planes[2].v != 1)
    return fail(MDCT_INVALID_PARAMETER, "chroma sampling factors %dx%d / %dx%d (1x1)", planes[1].h, planes[1].v, planes[2].h, planes[2].v);
  if (!((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2)))
    return fail(MDCT_INVALID_PARAMETER, "luma sampling factors %dx%d (1x1, 2x1 or 2x2)", h, v);
  const size_t mcus_x = planes[1].width / 8, mcus_y = planes[1].height / 8;
  for (int c = 0; c < 3; c++)
  {
    const mdct_jpegenc_scan_plane &p = planes[c];
    if (p.width == 0 || p.height == 0 || p.width > 65536 || p.height > 65536 || p.width != mcus_x * 8 * (size_t)p.h || p.height != mcus_y * 8 * (size_t)p.v)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: %zux%zu at sampling %dx%d is not on the MCU grid of %zux%zu MCUs the chroma planes state (width = mcus_x * 8 * h, "
                  "height = mcus_y * 8 * v, 8..65536)", c, p.width, p.height, p.h, p.v, mcus_x, mcus_y);
    if (p.pitch < p.width)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: pitch %zu < width %zu", c, p.pitch, p.width);
  }
  if (my0 >= my1 || my1 > mcus_y)
    return fail(MDCT_INVALID_PARAMETER, "MCU rows [%zu, %zu) of %zu", my0, my1, mcus_y);
  const int bpm = h * v + 2;
  const size_t need = mdct_jpegenc_scan_seg_stride(mcus_x, bpm);
  if (seg_stride < need || seg_stride % 4 != 0 || ((uintptr_t)out & 3))
    return fail(MDCT_INVALID_PARAMETER, "seg_stride %zu: a multiple of 4 and >= 208 * %zu blocks per MCU row + 8 = %zu (worst case of F.1.2); out 4-byte aligned",
                seg_stride, mcus_x * (size_t)bpm, need);
  ScanArgs a;
  memset(&a, 0, sizeof(a));
  const float *luts[2] = {lut_luma, lut_chroma};
  for (int t = 0; t < 2; t++)
  {
    const int bad = mdct::own_tables_fill(luts[t], a.tb[t], /*pair_order=*/true);
    if (bad >= 0)
      return fail(MDCT_INVALID_PARAMETER, "%s table entry %d is %g; finite non-zero entries", t ? "chroma" : "luma", bad, (double)luts[t][bad]);
  }
  const HuffCodes &hc = huff_codes();
  if (!hc.ok)
    return fail(MDCT_NOT_SUPPORTED, "mdct_huffman_spec failed");
  memcpy(a.dc, hc.dc, sizeof(a.dc));
  memcpy(a.ac, hc.ac, sizeof(a.ac));
  for (int c = 0; c < 3; c++)
  {
    a.px[c] = planes[c].px;
    a.pitch[c] = planes[c].pitch;
  }
  a.out = out;
  a.seg_bytes = seg_bytes;
  a.ff_counts = ff_counts;
  a.seg_stride = seg_stride;
  a.consts = mdct::DctConsts();
  a.mcus_x = (uint32_t)mcus_x;
  a.my0 = (uint32_t)my0;
  a.dc_shift = 64.0f * 128.0f;
  const dim3 grid((unsigned)(my1 - my0));
  const hipStream_t s = (hipStream_t)stream;
  if (h == 1)
    MDCT_LAUNCH((k_scan_rows<1, 1>), grid, dim3(64 * kWaves<1, 1>), 0, s, a);
  else if (v == 1)
    MDCT_LAUNCH((k_scan_rows<2, 1>), grid, dim3(64 * kWaves<2, 1>), 0, s, a);
  else
    MDCT_LAUNCH((k_scan_rows<2, 2>), grid, dim3(64 * kWaves<2, 2>), 0, s, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : fail(MDCT_NOT_SUPPORTED, "launch: %s", hipGetErrorString(e));
}

} // extern "C"
