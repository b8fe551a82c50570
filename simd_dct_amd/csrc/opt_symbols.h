// opt_symbols.h -- the kernel body of the chunked coders that take the caller's Huffman tables, and of their statistics form: k_opt
// (jpeg_encode_opt.hip, levels from pixels: ScanChunks) and k_coef (jpeg_coef.hip, levels from a coefficient plane: CoefChunks).  The
// source of the levels is the template parameter Chunks (scan_chunks.h); everything else exists once, here: the LDS, the table / ring /
// histogram set-up, the symbols phase (the histogram with its ballots, the walk that counts symbols without a code, HuffSeqCoder16)
// and the epilogue.
// Args: the kernel's argument struct with out, seg_stride, seg_bytes, ff_counts, hist, uncoded, mcus_x, my0, cls0, complete, dc[2][12]
// and ac[2][256] -- and, where Chunks::kCountsLoss, unrepresentable: a device word that takes the levels the source had to clamp
// (chunks.lost, counted by the lane that fetched the block) and the DC differences outside +-2047 (counted here, where they are known).
// Include after scan_chunks.h.  Device code only.
#pragma once
#include "huffman_rows.h"
#include "scan_chunks.h"
#include "wg_sync.h"

namespace mdct
{
namespace opt_symbols
{

constexpr uint32_t kRing = 1024;  // words of bit stream held in LDS (as k_scan_rows)
constexpr uint32_t kClass = 272;  // counts per class (MDCT_JPEGENC_OPT_HIST_CLASS)
constexpr uint32_t kHist = 2 * kClass;

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

// <H, V>: scan_order.h.  STATS = false: the symbols phase is HuffSeqCoder16 with the caller's tables; unless the host found the tables
// complete, a walk before it counts the symbols that have no code.  STATS = true: the symbols phase counts instead of coding.
template <class Chunks, int H, int V, bool STATS, class Args>
__device__ __forceinline__ void opt_kernel_body(const Args &a)
{
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
  [[maybe_unused]] uint32_t dc_lost = 0; // Chunks::kCountsLoss: DC differences outside +-2047 (known only here)
  wg_sync(); // tables and the cleared ring / histograms
  for (uint32_t m0 = 0, chunk = 0; m0 < a.mcus_x; m0 += M, chunk++)
  {
    chunks.transform(m0, chunk, par);
    wg_sync(); // every block of the chunk is in LDS
    const ChunkBlock b = chunks.block(sb, m0, par);
    const bool live = b.live, blk_eob = b.eob;
    const int blk_dc = b.dc, pred = b.pred, blk_n = live ? b.n : 0;
    if constexpr (Chunks::kCountsLoss)
      dc_lost += (live && (blk_dc - pred > 2047 || blk_dc - pred < -2047)) ? 1u : 0u;
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
  if constexpr (Chunks::kCountsLoss)
  {
    const uint32_t lost = chunks.lost + dc_lost;
    if (lost)
      atomicAdd(a.unrepresentable, lost);
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

} // namespace opt_symbols
} // namespace mdct
