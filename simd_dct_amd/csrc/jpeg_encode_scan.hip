// jpeg_encode_scan.hip -- the three component planes of a colour JPEG encode -> the Huffman segments of ONE INTERLEAVED scan
// (include/mdct_jpegenc_scan.h; ITU-T T.81 A.2.3), one segment per MCU row.
//
// Built into its own library, libmdct_jpegenc_scan.so, linked against libmdct_hip.so (launch tally, Huffman specifications).  The
// coefficients are the engine's own: the forward passes, the quantiser and the zig-zag compaction are aan_passes.h's and the multiplier
// tables own_tables.h's -- the code k_px_huffman_rows and mdct_fwd_u8_i16 are built from, not a restatement.
//
// One kernel template, k_scan_rows<H, V> (luma sampling; chroma is 1x1): 4:2:0 <2, 2>, 4:2:2 <2, 1>, 4:4:4 <1, 1>.  One workgroup per
// MCU row; the row is worked through in chunks of kMcus MCUs = 64 * kWaves blocks, each in a transform and a coding phase separated by
// a barrier.  The layouts and the scan order are scan_order.h's, the transform phase and the read-out of a thread's block in scan
// order scan_chunks.h's: both are shared with k_opt (jpeg_encode_opt.hip).  This kernel's own are the LDS, the Annex K tables and the
// bit-stream ring, the coding phase (HuffSeqCoder16, huffman_rows.h) and the epilogue.  The host checks it shares with
// jpeg_encode_opt.hip, and the Annex K codes it shares with jpeg_encode_batch.hip, are scan_host.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "aan_passes.h" // aan_fwd_h, aan_fwd_v, fwd_v_quant_levels, compact_levels16
#include "host_error.h"
#include "launch_tally.h"
#include "mdct_jpegenc_scan.h"
#include "scan_chunks.h"
#include "scan_host.h"
#include "wg_sync.h"

#pragma clang fp contract(off)

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

using namespace scan_order;

template <int H, int V>
__global__ __launch_bounds__((64 * kWaves<H, V>)) void k_scan_rows(ScanArgs a)
{
  using Chunks = ScanChunks<H, V, ScanArgs>;
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
  Chunks chunks(a);
  chunks.init(tid, lane, wave, my, rec_all, meta);

  // ---- the coding phase's block of this thread
  const SeqBlock sb = seq_block<H, V>(tid);
  const uint16_t *crec = rec_all + sb.slot * kRec16Row;
  const uint32_t *cac = ac[sb.chroma ? 1 : 0], *cdc = dc[sb.chroma ? 1 : 0];
  uint32_t par = 0;
  wg_sync(); // tables and the cleared ring
  for (uint32_t m0 = 0, chunk = 0; m0 < a.mcus_x; m0 += M, chunk++)
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
    a.seg_bytes[my] = coder.finish(&ff_last);
    a.ff_counts[my] = ff_total + ff_last;
  }
}

} // namespace jpegenc_scan
} // namespace mdct

using namespace mdct::jpegenc_scan;

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
  int h, v;
  size_t mcus_x, mcus_y;
  int rc = check_mcu_planes(planes, &h, &v, &mcus_x, &mcus_y);
  if (rc)
    return rc;
  if (my0 >= my1 || my1 > mcus_y)
    return fail(MDCT_INVALID_PARAMETER, "MCU rows [%zu, %zu) of %zu", my0, my1, mcus_y);
  const int bpm = h * v + 2;
  if ((rc = check_seg_stride(seg_stride, out, mdct_jpegenc_scan_seg_stride(mcus_x, bpm), 208, mcus_x * (size_t)bpm, "MCU row", "worst case of F.1.2")))
    return rc;
  ScanArgs a;
  memset(&a, 0, sizeof(a));
  if ((rc = fill_lut(lut_luma, a.tb[0], "luma")) || (rc = fill_lut(lut_chroma, a.tb[1], "chroma")))
    return rc;
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
