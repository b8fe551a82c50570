// jpeg_progressive.hip -- the scans of a progressive JPEG, spectral selection and successive approximation (include/mdct_jpegprog.h;
// ITU-T T.81 Annex G.1.2; DESIGN.md sections 4.12 and 4.12.1): quantised coefficient planes -> the segments of DC scans and of the scans
// of one AC band of one component with end-of-band runs, first scans and refinement scans, and their symbol statistics.
//
// Built into its own library, libmdct_jpegprog.so, linked against libmdct_hip.so (launch tally) and libmdct_jpegenc_opt.so (segment
// stride).
//
// k_prog_dc<H, V, STATS> is k_coef (jpeg_coef.hip) with a source that fetches the DC level alone: the kernel body is opt_symbols.h's
// with no AC entries and no EOB (HuffSeqCoder16::chunk with n = 0), the lane-to-block layout scan_chunks.h's ChunkGrid.
//
// k_prog_dc<H, V, false> with DcArgs' refine set is the DC refinement scan instead (dc_refine: one raw bit per block).
//
// k_prog_ac<STATS> branches, uniformly, into a first scan without or with a point transform (band_first) and a refinement scan
// (band_refine, described there); the kernels' names and number are those of the Ah = Al = 0 library.  A first scan:
// one workgroup of 4 waves per block row, chunks of 256 blocks, lane = block in both phases.
//   fetch    the lane's 8 rows (the fetch of CoefChunks), the levels of zig-zag positions ss..se compacted into its LDS row as
//            run << 12 | level entries; zeros outside the band are not counted and levels outside it do not appear.  Two flags per
//            block: non-empty (an entry) and tail (position se is zero); each wave leaves its two 64-bit ballots in LDS.
//   EOB run  the run pending before a non-empty block, and the ordinal of a tail block in its stretch, follow from the nearest
//            non-empty block before it: found in the wave's own mask, else in the earlier waves' masks, else the stretch began
//            before the chunk and the count carried in (uniform over the workgroup, kept mod 32767) is added.  No lane waits for
//            another.  A non-empty block codes EOBn of (pending mod 32767) in front of its entries; the tail block whose ordinal
//            reaches 32767 codes the full run (0xE0 and 14 one-bits) itself.
//   symbols  the token's bits join the lane's bit count; the scan of the counts, the ring, the 0xFF count and finish are
//            RingWriter's (huffman_rows.h; BandCoder below).  After the last chunk one lane writes the run still pending.
// What the scan kinds share around their middles -- set-up, fetch, unpacking, the histogram of entries, the epilogues -- is BandRow.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "aan_passes.h" // of it, compact_levels16 (k_prog_dc, through ChunkGrid) and kZigZag
#include "host_error.h"
#include "coef_host.h"
#include "launch_tally.h"
#include "mdct_jpegprog.h"
#include "scan_chunks.h"
#include "opt_symbols.h"
#include "scan_host.h"
#include "wg_sync.h"

namespace mdct
{
namespace jpegprog
{

using namespace scan_order;
using opt_symbols::kRing;

// ---------------------------------------------------------------------------------------------------------------------- the DC scan
struct DcArgs
{
  const int16_t *coef[3];
  size_t pitch[3]; // elements
  uint8_t *out;    // segments, seg_stride apart, indexed by the interval
  uint32_t *seg_bytes, *ff_counts;
  uint32_t *hist;            // STATS: [2][272]
  uint32_t *uncoded;         // coder: symbols without a code
  uint32_t *unrepresentable; // DC differences that had to be clamped
  size_t seg_stride;
  uint32_t mcus_x, my0;
  uint32_t cls0;       // one plane: its class in the histogram
  uint32_t complete;   // coder: every DC category has a code
  uint32_t al;         // the point transform: the scan codes dc >> al (arithmetic)
  uint32_t refine;     // coder: the refinement scan -- bit al of every DC, no table (dc_refine below)
  uint32_t dc[2][12];  // size << 16 | code per DC category, 0: no code; one plane: its table in [0]
  uint32_t ac[2][256]; // all zero: the body's AC tables, never looked up
};
static_assert(sizeof(DcArgs) <= 4096, "kernel argument block");

// The DC source of the chunk skeleton (scan_chunks.h): one 16-bit load per block.
template <int H, int V, class Args>
struct DcChunks : ChunkGrid<H, V, Args>
{
  using Grid = ChunkGrid<H, V, Args>;
  using Grid::a;
  using Grid::bx0;
  using Grid::last_blk;
  using Grid::M;
  using Grid::meta;
  using Grid::step;
  using Grid::tid;
  static constexpr bool kCountsLoss = true;

  const int16_t *src_row;
  int16_t level;
  uint32_t lost = 0; // no AC level is read

  __device__ __forceinline__ explicit DcChunks(const Args &a_) : Grid(a_) {}

  __device__ __forceinline__ void fetch(uint32_t bx) { level = (int16_t)(src_row[(size_t)min(bx, last_blk) * 8] >> a.al); }

  __device__ __forceinline__ void init(uint32_t tid_, uint32_t lane, uint32_t wave, uint32_t my, uint16_t *rec_all, uint32_t (*meta_)[Grid::kThreads])
  {
    uint32_t comp, brow;
    bool chroma_wave;
    Grid::place(tid_, lane, wave, my, rec_all, meta_, comp, brow, chroma_wave);
    const size_t pitch0 = a.pitch[0], pitch1 = a.pitch[1], pitch2 = a.pitch[2];
    const int16_t *const c0 = a.coef[0], *const c1 = a.coef[1], *const c2 = a.coef[2];
    src_row = (comp == 0 ? c0 : comp == 1 ? c1 : c2) + (size_t)brow * 8 * (comp == 0 ? pitch0 : comp == 1 ? pitch1 : pitch2);
    fetch(bx0);
  }

  // the DC level alone in meta[par][tid]: no entries, no EOB; then the next chunk's level is requested
  __device__ __forceinline__ void transform(uint32_t m0, uint32_t chunk, uint32_t par)
  {
    meta[par][tid] = (uint32_t)(uint16_t)level;
    if (m0 + M < a.mcus_x)
      fetch(bx0 + (chunk + 1) * step);
  }
};

// ---------------------------------------------------------------------------------------------------------------------- an AC band
struct BandArgs
{
  const int16_t *coef;
  size_t pitch; // elements
  uint8_t *out;
  uint32_t *seg_bytes, *ff_counts;
  uint32_t *hist; // STATS: [256]
  uint32_t *uncoded, *unrepresentable;
  size_t seg_stride;
  uint32_t blocks_x, by0;
  uint32_t ss, se;
  uint32_t complete; // coder: every symbol of a band scan has a code
  uint32_t ah, al;   // successive approximation: ah = 0, a first scan of |v| >> al with v's sign; ah = al + 1, the refinement scan of bit al of |v|
  uint32_t ac[256];  // size << 16 | code per RRRRSSSS, 0: no code
};
static_assert(sizeof(BandArgs) <= 4096, "kernel argument block");

constexpr uint32_t kBandWaves = 4, kBandThreads = 64 * kBandWaves;
constexpr uint32_t kFullRun = 0x7FFF; // the run that is emitted at once (EOB14 with 14 one-bits)

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// an end-of-band run 1..32767 -> RRRRSSSS = n << 4, and the n low bits of the run that follow the code
__device__ __forceinline__ void eob_run_symbol(uint32_t run, uint32_t &sym, uint32_t &extra, uint32_t &n)
{
  n = 31u - (uint32_t)__builtin_clz(run);
  sym = n << 4;
  extra = run & ((1u << n) - 1u);
}

// The run after block I of the chunk (0 where that block is no tail block; I = -1: the run carried in), not yet reduced mod 32767:
// ne / tl are the waves' ballots of non-empty and tail blocks.
__device__ __forceinline__ uint32_t run_after(int I, uint32_t carry, const unsigned long long *ne, const unsigned long long *tl)
{
  if (I < 0)
    return carry;
  int w = I >> 6;
  unsigned long long m = ne[w] & (~0ull >> (63 - (I & 63)));
#pragma unroll
  for (int k = 0; k < (int)kBandWaves - 1; k++)
    if (m == 0 && w > 0)
      m = ne[--w];
  if (m == 0)
    return carry + (uint32_t)I + 1u;
  const int j = 63 - __builtin_clzll(m);
  return (uint32_t)(I - (w * 64 + j)) + (uint32_t)((tl[w] >> j) & 1ull);
}

using BandWriter = RingWriter<(int)kBandWaves, kRing>;

// The coder of a first scan's chunk: no DC token; an optional run token (code of `sym`, then n_extra bits) in front of the lane's
// entries, no EOB behind them.
struct BandCoder : BandWriter
{
  __device__ __forceinline__ void chunk_band(const uint16_t *rec, int n, bool live, bool has_run, uint32_t sym, uint32_t extra, uint32_t n_extra, const uint32_t *ac)
  {
    const uint32_t *rec2 = reinterpret_cast<const uint32_t *>(rec);
    const uint32_t run_code = ac[sym & 0xFFu];
    uint32_t bits = 0;
    if (live)
    {
      if (has_run)
        bits = (run_code >> 16) + n_extra;
      bits += huff_count16(rec2, n, ac);
    }
    write(bits, live, [&](auto &put) {
      if (has_run)
      {
        put(run_code & 0xFFFFu, run_code >> 16);
        put(extra, n_extra);
      }
      huff_put16(put, rec2, n, ac);
    });
  }

  // one thread, after the last chunk (behind a workgroup barrier) and before finish: the run still pending, at most 16 + 14 bits.  The
  // ring's slot of the last, incomplete word holds its bits and the slot after it is clear.
  __device__ __forceinline__ void flush_run(uint32_t code, uint32_t extra, uint32_t n_extra)
  {
    const unsigned long long tok = (unsigned long long)(code & 0xFFFFu) << n_extra | extra;
    const uint32_t len = (code >> 16) + n_extra, wi = base_bits >> 5, off = base_bits & 31;
    if (len == 0)
      return;
    unsigned long long two = (unsigned long long)ring[wi & (kRing - 1)] << 32 | ring[(wi + 1) & (kRing - 1)];
    two |= tok << (64 - off - len); // off + len <= 31 + 30
    ring[wi & (kRing - 1)] = (uint32_t)(two >> 32);
    ring[(wi + 1) & (kRing - 1)] = (uint32_t)two;
    base_bits += len;
    if ((base_bits >> 5) > wi)
    { // the word is complete
      const uint32_t v = (uint32_t)(two >> 32);
      ff += (uint32_t)__builtin_popcount(ff_bytes(v));
      out_w[wi] = __builtin_bswap32(v);
    }
  }
};

constexpr uint32_t kBufWords = 32; // the buffer of a refinement scan's open run: 1024 bits >= 937 + 63

// the LDS of k_prog_ac<STATS>, one set for the scan kinds it branches into
template <bool STATS>
struct BandLds
{
  __attribute__((aligned(16))) uint16_t rec_all[kBandThreads * kRec16Row];
  uint32_t ac[STATS ? 1 : 256];
  unsigned long long ne[kBandWaves], tl[kBandWaves]; // the waves' ballots of non-empty and of tail blocks
  uint32_t ring[STATS ? 1 : kRing];
  uint32_t tot[2][kBandWaves];
  uint32_t ff_total;
  uint32_t hist[STATS ? kBandWaves : 1][STATS ? 256 : 1]; // one histogram per wave
  // a refinement scan only
  uint32_t info[kBandThreads];                        // non-empty | tail << 1 | tail bits << 2
  uint32_t buf[STATS ? 1 : 2][STATS ? 1 : kBufWords]; // the tail bits of the open run, MSB first; the other one is clear
};

// What the scan kinds of a band share, around a coder of the scan's kind: the set-up of LDS and of the segment, the lane's block (its
// 8 rows streamed into registers one chunk ahead, unpacked to 64 levels), the histogram of the lanes' entries and the epilogues.
template <bool STATS, class Coder>
struct BandRow
{
  const BandArgs &a;
  BandLds<STATS> &lds;
  uint32_t tid, lane, wave, by, last_blk;
  uint16_t *rec;   // the lane's LDS row
  uint32_t *whist; // STATS: the wave's histogram
  const int16_t *src_row;
  size_t pitch;
  uint4 rows[8];
  Coder coder;

  // ends with the first chunk's rows requested; the caller's barrier publishes the table and the cleared ring / histograms
  __device__ __forceinline__ BandRow(const BandArgs &a_, BandLds<STATS> &lds_) : a(a_), lds(lds_)
  {
    tid = threadIdx.x;
    lane = tid & 63;
    wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    by = a.by0 + blockIdx.x;
    last_blk = a.blocks_x - 1;
    if constexpr (STATS)
    {
      for (uint32_t i = tid; i < kBandWaves * 256; i += kBandThreads)
        (&lds.hist[0][0])[i] = 0;
    }
    else
    {
      lds.ac[tid] = a.ac[tid];
      if (tid == 0)
        lds.ff_total = 0;
      for (uint32_t w = tid; w < kRing; w += kBandThreads)
        lds.ring[w] = 0;
      coder.ring = lds.ring;
      coder.tot = lds.tot;
      coder.out_w = reinterpret_cast<uint32_t *>(a.out + (size_t)by * a.seg_stride);
    }
    rec = lds.rec_all + tid * kRec16Row;
    whist = lds.hist[STATS ? wave : 0];
    pitch = a.pitch;
    src_row = a.coef + (size_t)by * 8 * pitch;
    fetch(tid);
  }

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

  // the fetched block's 64 levels in raster order
  __device__ __forceinline__ void unpack(int (&val)[64]) const
  {
#pragma unroll
    for (int r = 0; r < 8; r++)
    {
      const uint32_t w[4] = {rows[r].x, rows[r].y, rows[r].z, rows[r].w};
#pragma unroll
      for (int u = 0; u < 8; u++)
        val[r * 8 + u] = (u & 1) ? (int)w[u >> 1] >> 16 : (int)(int16_t)(w[u >> 1] & 0xFFFFu);
    }
  }

  // STATS: the symbols sym(i) of the lane's n entries join the wave's histogram, the lanes' i-th entries together; s0, s1, s2 are
  // symbols that many lanes hold at once: one add per wave (template parameters: as function arguments they cost the refinement
  // scan's statistics 4 %)
  template <uint32_t s0, uint32_t s1, uint32_t s2, class Sym>
  __device__ __forceinline__ void count_entries(int n, Sym sym)
  {
    auto add_ballot = [&](bool p, uint32_t s) {
      const uint32_t c = (uint32_t)__popcll(__ballot(p));
      if (lane == 0 && c)
        atomicAdd(&whist[s], c);
    };
    for (int i = 0; __ballot(i < n) != 0; i++)
    {
      const bool on = i < n;
      const uint32_t s = on ? sym(i) : 0xFFFFu;
      add_ballot(s == s0, s0);
      add_ballot(s == s1, s1);
      add_ballot(s == s2, s2);
      if (on && s != s0 && s != s1 && s != s2)
        atomicAdd(&whist[s], 1u);
    }
  }

  // STATS, after the last chunk: the waves' histograms join the caller's
  __device__ __forceinline__ void sum_hist()
  {
    wg_sync();
    uint32_t s = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBandWaves; w++)
      s += lds.hist[w][tid];
    if (s)
      atomicAdd(&a.hist[tid], s);
  }

  // the coder, after the last chunk: the segment's padded end, its length and its 0xFF count
  __device__ __forceinline__ void finish()
  {
    if (coder.ff)
      atomicAdd(&lds.ff_total, coder.ff);
    wg_sync();
    if (tid == 0)
    {
      uint32_t ff_last;
      a.seg_bytes[by] = coder.finish(&ff_last);
      a.ff_counts[by] = lds.ff_total + ff_last;
    }
  }
};

// A first scan (Ah = 0).  SHIFT: Al > 0 -- the level is |v| >> al with v's sign (clamped first); a level that becomes 0 is a zero for
// runs and tail flag alike
template <bool STATS, bool SHIFT>
__device__ __forceinline__ void band_first(const BandArgs &a, BandLds<STATS> &lds)
{
  BandRow<STATS, BandCoder> row(a, lds);
  auto &ac = lds.ac;
  auto &ne = lds.ne;
  auto &tl = lds.tl;
  const uint32_t tid = row.tid, lane = row.lane, wave = row.wave;
  const uint32_t ss = a.ss, se = a.se, last_blk = row.last_blk;
  uint16_t *rec = row.rec;
  uint32_t *whist = row.whist;
  uint32_t carry = 0; // the run pending after the chunks so far, mod 32767; uniform
  uint32_t lost = 0, uncoded = 0;
  wg_sync(); // the table and the cleared ring / histograms
  for (uint32_t m0 = 0; m0 < a.blocks_x; m0 += kBandThreads)
  {
    const bool live = m0 + tid <= last_blk;
    // ---- levels of the band -> entries (compact_levels16 with the band's bounds; AC clamped to +-1023 and counted)
    int val[64];
    row.unpack(val);
    uint32_t pos = 0, r12 = 0, clamped = 0;
    bool se_coded = false;
#pragma unroll
    for (int k = 1; k < 64; k++)
    {
      const bool in = (uint32_t)k >= ss && (uint32_t)k <= se;
      const int l = val[kZigZag[k]];
      int c = l > 1023 ? 1023 : (l < -1023 ? -1023 : l);
      clamped += (in && c != l) ? 1u : 0u;
      if constexpr (SHIFT)
      {
        const int mag = (c < 0 ? -c : c) >> a.al;
        c = c < 0 ? -mag : mag;
      }
      const bool nz = in && c != 0;
      const bool wr = nz || (in && r12 == 0xF000u);
      rec[pos] = (uint16_t)(((uint32_t)c & 0xFFFu) | r12);
      pos += wr ? 1u : 0u;
      r12 = wr ? 0u : (in ? r12 + 0x1000u : r12);
      se_coded = se_coded || ((uint32_t)k == se && nz);
    }
    uint32_t n_all = pos;
#pragma unroll
    for (int t = 0; t < 3; t++) // ZRL entries after the last level become part of the end of band
      n_all -= (n_all > 0 && rec[n_all - 1] == 0xF000u) ? 1u : 0u;
    const int n = live ? (int)n_all : 0;
    lost += live ? clamped : 0u;
    const bool nonempty = n > 0, tail = live && !se_coded;
    const unsigned long long bne = __ballot(nonempty), btl = __ballot(tail);
    if (lane == 0)
    {
      ne[wave] = bne;
      tl[wave] = btl;
    }
    if (m0 + kBandThreads < a.blocks_x)
      row.fetch(m0 + kBandThreads + tid);
    wg_sync(); // the ballots of every wave
    // ---- the end-of-band run in front of this block
    const uint32_t r = run_after(nonempty ? (int)tid - 1 : (int)tid, carry, ne, tl);
    const uint32_t r_end = run_after((int)min(kBandThreads - 1, last_blk - m0), carry, ne, tl);
    bool has_run = false;
    uint32_t sym = 0, extra = 0, n_extra = 0;
    if (nonempty)
    {
      const uint32_t p = r >= kFullRun ? r - kFullRun : r;
      has_run = p != 0;
      if (has_run)
        eob_run_symbol(p, sym, extra, n_extra);
    }
    else if (live && r == kFullRun)
    {
      has_run = true;
      eob_run_symbol(kFullRun, sym, extra, n_extra);
    }
    carry = r_end >= kFullRun ? r_end - kFullRun : r_end;
    if constexpr (STATS)
    {
      if (has_run)
        atomicAdd(&whist[sym], 1u);
      row.template count_entries<0x01u, 0x02u, 0x11u>(n, [&](int i) { return opt_symbols::ac_symbol12(rec[i]); });
      wg_sync(); // every lane has read the ballots: the next chunk may write them (the coder's barriers)
    }
    else
    {
      if (!a.complete)
      { // the symbols this block needs that the table does not code
        if (has_run)
          uncoded += (ac[sym] >> 16) == 0 ? 1u : 0u;
        for (int i = 0; i < n; i++)
          uncoded += (ac[opt_symbols::ac_symbol12(rec[i])] >> 16) == 0 ? 1u : 0u;
      }
      row.coder.chunk_band(rec, n, live, has_run, sym, extra, n_extra, ac);
    }
  }
  // ---- the run still pending ends with the interval
  uint32_t sym = 0, extra = 0, n_extra = 0;
  if (carry)
    eob_run_symbol(carry, sym, extra, n_extra);
  if (lost)
    atomicAdd(a.unrepresentable, lost);
  if constexpr (STATS)
  {
    if (tid == 0 && carry)
      atomicAdd(&whist[sym], 1u);
    row.sum_hist();
  }
  else
  {
    if (tid == 0 && carry && !a.complete)
      uncoded += (ac[sym] >> 16) == 0 ? 1u : 0u;
    if (uncoded)
      atomicAdd(a.uncoded, uncoded);
    wg_sync(); // every wave has flushed and cleared the last chunk's words
    if (tid == 0 && carry)
      row.coder.flush_run(ac[sym], extra, n_extra); // a word it completes joins this thread's 0xFF count, added by finish
    row.finish();
  }
}

// ------------------------------------------------------------------------------------------------------- an AC refinement scan
// band_refine<STATS>, the Ah != 0 branch of k_prog_ac: libjpeg's encode_mcu_AC_refine in the first scan's shape -- one workgroup of 4 waves per block row, chunks of 256
// blocks, lane = block.  With a[k] = min(|v[k]|, 1023) >> al and EOB the last position of the band with a == 1, a block is
//   content  (only if some a == 1: the block is NON-EMPTY) per a == 1 the symbol r << 4 | 1 and a sign bit, and a ZRL at the 16th zero
//            in a row in front of EOB; behind either, the correction bits (a & 1 of the positions with a > 1) gathered since the last one;
//   tail     the correction bits behind EOB; the block is a TAIL block if any position follows EOB (always, if it is empty).
// A run is a stretch of tail blocks: it begins at a tail block (the only one that may be non-empty) and ends in front of the next
// non-empty block, behind the block that makes it 0x7FFF long or its tail bits more than 937, or with the interval.  The stream holds
// a run as EOBn, then the tail bits of its blocks in order, so the lane of the run's FIRST block emits the token once the run's
// length is known:
//   closed in this chunk   the length follows from the masks of non-empty and of flushing blocks; content, token and tail bits take
//                          their places through the scan of the lanes' bit counts;
//   open at the chunk's end   its tail bits go into an LDS buffer (at most 937 + 63 bits) that is carried with the run's length; the
//                          chunk that closes it has lane 0 emit the token and the buffer in front of everything else.
// The flush rule is a running sum with resets: every wave walks the chunk's 256 (non-empty, tail, tail bits) triples, read from LDS
// into four registers beforehand and taken by v_readlane, in scalar registers alone; it yields the mask of flushing blocks, the
// state after the chunk and where the run that stays open began.
constexpr uint32_t kMaxBuffered = 937; // libjpeg's MAX_CORR_BITS - DCTSIZE2 + 1: a run whose buffered bits exceed it is flushed
constexpr uint32_t kNone = 1024;       // "no such block" of next_block

// the first block >= from whose bit is set in the four 64-bit masks, or kNone
__device__ __forceinline__ uint32_t next_block(unsigned long long m0, unsigned long long m1, unsigned long long m2, unsigned long long m3, uint32_t from)
{
  const unsigned long long m[4] = {m0, m1, m2, m3};
  uint32_t res = kNone;
#pragma unroll
  for (int w = 3; w >= 0; w--)
  {
    const int lo = (int)from - w * 64;
    const unsigned long long x = lo >= 64 ? 0ull : (lo > 0 ? m[w] & (~0ull << lo) : m[w]);
    if (x)
      res = (uint32_t)(w * 64 + __builtin_ctzll(x));
  }
  return res;
}

__device__ __forceinline__ bool block_bit(unsigned long long m0, unsigned long long m1, unsigned long long m2, unsigned long long m3, uint32_t i)
{
  const uint32_t w = i >> 6;
  const unsigned long long m = w == 0 ? m0 : w == 1 ? m1 : w == 2 ? m2 : m3;
  return ((m >> (i & 63)) & 1ull) != 0;
}

// entries of a refinement block in its LDS row: symbol (r << 4 | 1, or 0xF0) | sign << 8 | correction bits behind it << 9
__device__ __forceinline__ uint32_t ref_symbol(uint32_t e) { return e & 0xFFu; }
__device__ __forceinline__ uint32_t ref_ncorr(uint32_t e) { return e >> 9; }

// A refinement lane's bits are a sequence only it can replay, and the writer scans two counts at once: the lane's bit count, and
// above kBitsMask the bits it leaves in the carried buffer (a chunk holds < 2^19 bits and an open run <= 1000 buffered ones).
constexpr uint32_t kBitsMask = 0xFFFFFu, kBufferedShift = 20;

// the low n <= 63 bits of v, most significant first, in pieces put takes
template <class Put>
__device__ __forceinline__ void put_bits64(Put &put, unsigned long long v, uint32_t n)
{
  while (n > 16)
  {
    n -= 16;
    put((uint32_t)(v >> n) & 0xFFFFu, 16);
  }
  put((uint32_t)v & ((1u << n) - 1u), n);
}

template <bool STATS>
__device__ __forceinline__ void band_refine(const BandArgs &a, BandLds<STATS> &lds)
{
  BandRow<STATS, BandWriter> row(a, lds);
  auto &coder = row.coder;
  auto &ac = lds.ac;
  auto &ne = lds.ne;
  auto &tl = lds.tl;
  auto &info = lds.info;
  auto &buf = lds.buf;
  const uint32_t tid = row.tid, lane = row.lane, wave = row.wave;
  const uint32_t ss = a.ss, se = a.se, al = a.al, last_blk = row.last_blk;
  uint16_t *rec = row.rec;
  uint32_t *whist = row.whist;
  if constexpr (!STATS)
  {
    if (tid < 2 * kBufWords)
      (&buf[0][0])[tid] = 0;
  }
  // the run pending after the chunks so far and its buffered bits (in buf[cur]); uniform
  uint32_t run_c = 0, be_c = 0, cur = 0;
  uint32_t uncoded = 0;
  wg_sync(); // the table and the cleared ring / buffers / histograms
  for (uint32_t m0 = 0; m0 < a.blocks_x; m0 += kBandThreads)
  {
    const bool live = m0 + tid <= last_blk;
    const bool last_chunk = m0 + kBandThreads >= a.blocks_x;
    const uint32_t n_live = min(kBandThreads, a.blocks_x - m0);
    // ---- the block's entries, correction bits and flags
    int val[64];
    row.unpack(val);
    auto level = [&](int l) { // a[k]: the clamp first, so every scan of a coefficient sees one value
      const int m = l < 0 ? -l : l;
      return (uint32_t)(m > 1023 ? 1023 : m) >> al;
    };
    // A ZRL is written at every 16th zero; those behind the last a == 1 (EOB) are dropped afterwards, as k_prog_ac drops them, and
    // what they held of correction bits is tail: `keep` entries and `used` bits stand in front of EOB's end.
    uint32_t pos = 0, r = 0, br = 0, ncb = 0, keep = 0, used = 0;
    bool se_one = false;
    unsigned long long cb = 0; // the block's correction bits in order, the first one most significant of the ncb
#pragma unroll
    for (int k = 1; k < 64; k++)
    {
      const bool in = (uint32_t)k >= ss && (uint32_t)k <= se;
      const int l = val[kZigZag[k]];
      const uint32_t av = level(l);
      const bool zero = in && av == 0, one = in && av == 1, big = in && av > 1;
      const uint32_t r_new = zero ? r + 1 : r;
      const bool zrl = zero && r_new == 16;
      const bool wr = one || zrl;
      rec[pos] = (uint16_t)((one ? (r << 4 | 1u | (l > 0 ? 0x100u : 0u)) : 0xF0u) | br << 9);
      pos += wr ? 1u : 0u;
      br = wr ? 0u : (big ? br + 1 : br);
      r = wr ? 0u : r_new;
      cb = big ? (cb << 1 | (av & 1u)) : cb;
      ncb += big ? 1u : 0u;
      keep = one ? pos : keep;
      used = one ? ncb : used;
      se_one = se_one || ((uint32_t)k == se && one);
    }
    const int n = live ? (int)keep : 0;
    const bool nonempty = live && keep != 0, tail = live && !se_one;
    const uint32_t tb = tail ? ncb - used : 0u;
    const unsigned long long bne = __ballot(nonempty), btl = __ballot(tail);
    if (lane == 0)
    {
      ne[wave] = bne;
      tl[wave] = btl;
    }
    info[tid] = (nonempty ? 1u : 0u) | (tail ? 2u : 0u) | tb << 2;
    if (!last_chunk)
      row.fetch(m0 + kBandThreads + tid);
    wg_sync(); // the ballots and the triples of every wave
    // ---- the flush rule: every wave walks the chunk, in scalar registers
    uint32_t iv[kBandWaves];
#pragma unroll
    for (uint32_t w = 0; w < kBandWaves; w++)
      iv[w] = info[w * 64 + lane];
    unsigned long long fl[kBandWaves];
    uint32_t run = run_c, be = be_c;
    int open_at = -1; // where the run that is open began; -1: before this chunk
#pragma unroll
    for (uint32_t w = 0; w < kBandWaves; w++)
    {
      unsigned long long f = 0;
      for (uint32_t j = 0; j < 64; j++)
      {
        const uint32_t x = (uint32_t)__builtin_amdgcn_readlane((int)iv[w], (int)j);
        if (x & 1u)
          run = be = 0;
        if (x & 2u)
        {
          open_at = run == 0 ? (int)(w * 64 + j) : open_at;
          run++;
          be += x >> 2;
          if (run == kFullRun || be > kMaxBuffered)
          {
            f |= 1ull << j;
            run = be = 0;
          }
        }
      }
      fl[w] = f;
    }
    if (last_chunk)
      run = be = 0; // the interval's end closes the run: nothing stays open
    const unsigned long long ne0 = ne[0], ne1 = ne[1], ne2 = ne[2], ne3 = ne[3];
    const unsigned long long tl0 = tl[0], tl1 = tl[1], tl2 = tl[2], tl3 = tl[3];
    const uint32_t end_close = last_chunk ? n_live : kNone;
    // where the run that holds block `from` as a tail block ends: in front of the next non-empty block behind `from`, behind the
    // next flushing block, or with the interval; kNone: not in this chunk
    auto close_of = [&](uint32_t from_ne, uint32_t from_fl) {
      const uint32_t c_ne = next_block(ne0, ne1, ne2, ne3, from_ne);
      const uint32_t c_fl = next_block(fl[0], fl[1], fl[2], fl[3], from_fl);
      return min(min(c_ne, c_fl == kNone ? kNone : c_fl + 1), end_close);
    };
    // ---- this lane's tokens
    // lane 0: the run carried in, if it ends here
    bool pre = false;
    uint32_t pre_sym = 0, pre_extra = 0, pre_n = 0;
    if (tid == 0 && run_c != 0)
    {
      const uint32_t c0 = close_of(0, 0);
      if (c0 != kNone)
      {
        pre = true;
        eob_run_symbol(run_c + c0, pre_sym, pre_extra, pre_n);
      }
    }
    // a run that begins at this block
    bool starts = false;
    if (tail)
      starts = nonempty || (tid == 0 ? run_c == 0 : (block_bit(fl[0], fl[1], fl[2], fl[3], tid - 1) || !block_bit(tl0, tl1, tl2, tl3, tid - 1)));
    const bool in_open = tail && run != 0 && (int)tid >= open_at;
    bool has_run = false;
    uint32_t sym = 0, extra = 0, n_extra = 0;
    if (starts && !in_open)
    {
      has_run = true;
      eob_run_symbol(close_of(tid + 1, tid) - tid, sym, extra, n_extra);
    }
    const uint32_t tail_here = in_open ? 0u : tb; // tail bits emitted in place
    if constexpr (STATS)
    {
      if (pre)
        atomicAdd(&whist[pre_sym], 1u);
      if (has_run)
        atomicAdd(&whist[sym], 1u);
      row.template count_entries<0x01u, 0x11u, 0x21u>(n, [&](int i) { return ref_symbol(rec[i]); });
      wg_sync(); // every lane has read the ballots and its row: the next chunk may write them
    }
    else
    {
      // ---- the lane's bit count
      uint32_t bits = 0;
      if (pre)
      {
        bits += (ac[pre_sym] >> 16) + pre_n + be_c;
        uncoded += (ac[pre_sym] >> 16) == 0 ? 1u : 0u;
      }
      for (int i = 0; i < n; i++)
      {
        const uint32_t e = rec[i], len = ac[ref_symbol(e)] >> 16;
        bits += len + (ref_symbol(e) == 0xF0u ? 0u : 1u);
        uncoded += len == 0 ? 1u : 0u;
      }
      bits += (live ? used : 0u) + tail_here; // the correction bits in front of EOB's end, and the tail if it is emitted in place
      if (has_run)
      {
        bits += (ac[sym] >> 16) + n_extra;
        uncoded += (ac[sym] >> 16) == 0 ? 1u : 0u;
      }
      const uint32_t *rd = buf[cur];              // what lane 0 emits of the run carried in
      uint32_t *wr = buf[open_at < 0 ? cur : cur ^ 1u]; // where the open run's tail bits go: behind those carried, or into the clear buffer
      // a lane without bits writes nothing
      const uint32_t before = coder.template write<kBitsMask>(bits | (in_open ? tb : 0u) << kBufferedShift, live && bits, [&](auto &put) {
        if (pre)
        {
          const uint32_t code = ac[pre_sym];
          put(code & 0xFFFFu, code >> 16);
          put(pre_extra, pre_n);
          uint32_t w = 0;
          for (; w < (be_c >> 5); w++)
          {
            put(rd[w] >> 16, 16);
            put(rd[w] & 0xFFFFu, 16);
          }
          if (be_c & 31u)
            put_bits64(put, rd[w] >> (32 - (be_c & 31u)), be_c & 31u);
        }
        uint32_t left = ncb; // correction bits not yet emitted: the low `left` bits of cb
        for (int i = 0; i < n; i++)
        {
          const uint32_t e = rec[i], code = ac[ref_symbol(e)];
          put(code & 0xFFFFu, code >> 16);
          if (ref_symbol(e) != 0xF0u)
            put((e >> 8) & 1u, 1);
          const uint32_t nc = ref_ncorr(e);
          left -= nc;
          put_bits64(put, (cb >> left) & ((1ull << nc) - 1ull), nc);
        }
        if (has_run)
        {
          const uint32_t code = ac[sym];
          put(code & 0xFFFFu, code >> 16);
          put(extra, n_extra);
        }
        put_bits64(put, cb & ((1ull << tail_here) - 1ull), tail_here);
      }).before >> kBufferedShift;
      // ---- the open run's tail bits join the buffer (no lane reads that buffer in this chunk)
      if (in_open && tb)
      {
        uint32_t o = (open_at < 0 ? be_c : 0u) + before, left = tb;
        while (left)
        {
          const uint32_t room = 32 - (o & 31u), take = min(room, left);
          left -= take;
          atomicOr(&wr[(o >> 5) & (kBufWords - 1)], ((uint32_t)(cb >> left) & (uint32_t)((1ull << take) - 1ull)) << (room - take));
          o += take;
        }
      }
      if (run == 0 || open_at >= 0)
      { // the carried run has ended: its buffer is clear for the chunk after the next, the other one is current
        if (tid < kBufWords)
          buf[cur][tid] = 0;
        cur ^= 1u;
      }
    }
    run_c = run;
    be_c = be;
  }
  if constexpr (STATS)
    row.sum_hist();
  else
  {
    if (uncoded)
      atomicAdd(a.uncoded, uncoded);
    row.finish();
  }
}

// one kernel per table form, as the DC scan has: the scan kind is a uniform branch (one set of LDS, the registers of the widest)
// (two waves per SIMD, the occupancy of the Al = 0 branch on its own, hold for all three)
template <bool STATS>
__global__ __launch_bounds__(kBandThreads) __attribute__((amdgpu_waves_per_eu(2))) void k_prog_ac(BandArgs a)
{
  __shared__ BandLds<STATS> lds;
  if (a.ah != 0)
    band_refine<STATS>(a, lds);
  else if (a.al != 0)
    band_first<STATS, true>(a, lds);
  else
    band_first<STATS, false>(a, lds);
}

// --------------------------------------------------------------------------------------------------------- a DC refinement scan
// One raw bit (dc >> al) & 1 per block in scan order (G.1.2.1), a workgroup per interval, a thread per 32 blocks: no table, no
// statistics.  The last byte is padded with 1-bits.  The branch of k_prog_dc<H, V, false> that DcArgs' refine selects.
template <int H, int V>
__device__ __forceinline__ void dc_refine(const DcArgs &a)
{
  __shared__ uint32_t ff_total;
  constexpr uint32_t kThreads = 64 * kWaves<H, V>;
  const uint32_t tid = threadIdx.x, my = a.my0 + blockIdx.x;
  constexpr uint32_t h = H, hd = H ? H : 1, v = V, luma = h * v, per_mcu = h ? luma + 2 : 1;
  const uint32_t n_bits = a.mcus_x * per_mcu, n_bytes = (n_bits + 7) / 8, n_words = (n_bytes + 3) / 4;
  uint32_t *out_w = reinterpret_cast<uint32_t *>(a.out + (size_t)my * a.seg_stride);
  if (tid == 0)
    ff_total = 0;
  __syncthreads();
  uint32_t ff = 0;
  for (uint32_t w = tid; w < n_words; w += kThreads)
  {
    uint32_t word = 0;
    for (uint32_t b = 0; b < 32; b++)
    {
      const uint32_t i = w * 32 + b;
      uint32_t bit = 1;
      if (i < n_bits)
      {
        const uint32_t m = i / per_mcu, u = i - m * per_mcu;
        const bool chroma = h != 0 && u >= luma;
        const uint32_t comp = chroma ? 1 + (u - luma) : 0;
        const uint32_t row = (h == 0 || chroma) ? my : my * v + u / hd, col = (h == 0 || chroma) ? m : m * h + u % hd;
        const int16_t *p = comp == 0 ? a.coef[0] : comp == 1 ? a.coef[1] : a.coef[2];
        const size_t pitch = comp == 0 ? a.pitch[0] : comp == 1 ? a.pitch[1] : a.pitch[2];
        bit = ((uint32_t)((int)p[(size_t)row * 8 * pitch + (size_t)col * 8] >> a.al)) & 1u;
      }
      word = word << 1 | bit;
    }
    const uint32_t valid = min(4u, n_bytes - 4 * w); // the stream is MSB first: its bytes are the word's top ones
    ff += (uint32_t)__builtin_popcount(ff_bytes(word) & (0xFFFFFFFFu << (8 * (4 - valid))));
    out_w[w] = __builtin_bswap32(word);
  }
  if (ff)
    atomicAdd(&ff_total, ff);
  __syncthreads();
  if (tid == 0)
  {
    a.seg_bytes[my] = n_bytes;
    a.ff_counts[my] = ff_total;
  }
}

template <int H, int V, bool STATS>
__global__ __launch_bounds__((64 * kWaves<H, V>)) void k_prog_dc(DcArgs a)
{
  if constexpr (!STATS)
  {
    if (a.refine)
    {
      dc_refine<H, V>(a);
      return;
    }
  }
  opt_symbols::opt_kernel_body<DcChunks<H, V, DcArgs>, H, V, STATS>(a);
}

} // namespace jpegprog
} // namespace mdct

using namespace mdct::jpegprog;
using mdct::opt_symbols::kHist;

namespace
{

static_assert(mdct::opt_symbols::kClass == MDCT_JPEGENC_OPT_HIST_CLASS, "counts per class");

// the planes of a DC scan: one, or three on one MCU grid (the samplings mdct_jpegcoef_scan_rows takes); *h = 0: one plane
int check_dc_planes(const mdct_jpegcoef_plane *planes, int n_planes, int interleaved, int *h, int *v, uint32_t *per_row, uint32_t *n_rows)
{
  if (interleaved != 0 && interleaved != 1)
    return fail(MDCT_INVALID_PARAMETER, "interleaved %d (0 or 1)", interleaved);
  if (n_planes != (interleaved ? 3 : 1))
    return fail(MDCT_INVALID_PARAMETER, "%d planes (interleaved = 0 takes one, interleaved = 1 takes Y, Cb, Cr)", n_planes);
  if (interleaved)
    return check_coef_mcu_planes(planes, h, v, per_row, n_rows);
  *h = *v = 0;
  *per_row = planes[0].blocks_x;
  *n_rows = planes[0].blocks_y;
  return check_coef_plane(planes[0], "plane", 0);
}

int check_band(int ss, int se)
{
  if (ss < 1 || se > 63 || ss > se)
    return fail(MDCT_INVALID_PARAMETER, "band %d..%d (1 <= ss <= se <= 63)", ss, se);
  return MDCT_SUCCESS;
}

// the successive approximation of a scan: Al 0..13; Ah 0 (a first scan) or Al + 1 (the scan refines the one bit below its predecessor's Al)
int check_approx(int ah, int al)
{
  if (al < 0 || al > 13)
    return fail(MDCT_INVALID_PARAMETER, "successive approximation Al %d (0..13)", al);
  if (ah != 0 && ah != al + 1)
    return fail(MDCT_INVALID_PARAMETER, "successive approximation Ah %d with Al %d (Ah is 0 for a first scan, Al + 1 for a refinement scan)", ah, al);
  return MDCT_SUCCESS;
}

int launched()
{
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : fail(MDCT_NOT_SUPPORTED, "launch: %s", hipGetErrorString(e));
}

template <bool STATS>
int launch_dc(const DcArgs &a, int h, int v, unsigned n_intervals, hipStream_t s)
{
  const dim3 grid(n_intervals);
  if (h == 0)
    MDCT_LAUNCH((k_prog_dc<0, 0, STATS>), grid, dim3(64 * kWaves<0, 0>), 0, s, a);
  else if (h == 1)
    MDCT_LAUNCH((k_prog_dc<1, 1, STATS>), grid, dim3(64 * kWaves<1, 1>), 0, s, a);
  else if (v == 1)
    MDCT_LAUNCH((k_prog_dc<2, 1, STATS>), grid, dim3(64 * kWaves<2, 1>), 0, s, a);
  else
    MDCT_LAUNCH((k_prog_dc<2, 2, STATS>), grid, dim3(64 * kWaves<2, 2>), 0, s, a);
  return launched();
}

void dc_planes(DcArgs &a, const mdct_jpegcoef_plane *planes, int n_planes, uint32_t per_row)
{
  for (int c = 0; c < n_planes; c++)
  {
    a.coef[c] = planes[c].coef;
    a.pitch[c] = planes[c].pitch;
  }
  a.mcus_x = per_row;
}

void band_plane(BandArgs &a, const mdct_jpegcoef_plane &p, int ss, int se)
{
  a.coef = p.coef;
  a.pitch = p.pitch;
  a.blocks_x = p.blocks_x;
  a.ss = (uint32_t)ss;
  a.se = (uint32_t)se;
}

} // namespace

extern "C" {

const char *mdct_jpegprog_last_error(void) { return g_err; }

int mdct_jpegprog_dc_stats(const mdct_jpegcoef_plane *planes, int n_planes, int interleaved, int cls, uint32_t *hist, uint32_t *unrepresentable, void *stream)
{
  return mdct_jpegprog_dc_stats_approx(planes, n_planes, interleaved, cls, 0, 0, hist, unrepresentable, stream);
}

int mdct_jpegprog_dc_stats_approx(const mdct_jpegcoef_plane *planes, int n_planes, int interleaved, int cls, int ah, int al, uint32_t *hist, uint32_t *unrepresentable,
                                  void *stream)
{
  if (!planes || !hist || !unrepresentable)
    return fail(MDCT_INVALID_PARAMETER, "null planes / hist / unrepresentable");
  if (cls != 0 && cls != 1)
    return fail(MDCT_INVALID_PARAMETER, "class %d (0 luminance, 1 chrominance)", cls);
  int rc, h, v;
  uint32_t per_row, n_rows;
  if ((rc = check_approx(ah, al)))
    return rc;
  if (ah != 0)
    return fail(MDCT_INVALID_PARAMETER, "Ah %d: a DC refinement scan holds raw bits and has no symbols to count", ah);
  if ((rc = check_word(hist, "hist")) || (rc = check_word(unrepresentable, "unrepresentable")) || (rc = check_dc_planes(planes, n_planes, interleaved, &h, &v, &per_row, &n_rows)))
    return rc;
  DcArgs a;
  memset(&a, 0, sizeof(a));
  a.hist = hist;
  a.unrepresentable = unrepresentable;
  a.cls0 = (uint32_t)cls;
  a.al = (uint32_t)al;
  dc_planes(a, planes, n_planes, per_row);
  const hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(hist, 0, sizeof(uint32_t) * kHist, s);
  if (e != hipSuccess)
    return fail(MDCT_NOT_SUPPORTED, "memset: %s", hipGetErrorString(e));
  return launch_dc<true>(a, h, v, n_rows, s);
}

int mdct_jpegprog_dc_rows(const mdct_jpegcoef_plane *planes, int n_planes, int interleaved, const mdct_jpegenc_opt_spec *specs, size_t r0, size_t r1, uint8_t *out,
                          size_t seg_stride, uint32_t *seg_bytes, uint32_t *ff_counts, uint32_t *uncoded, uint32_t *unrepresentable, void *stream)
{
  return mdct_jpegprog_dc_rows_approx(planes, n_planes, interleaved, specs, 0, 0, r0, r1, out, seg_stride, seg_bytes, ff_counts, uncoded, unrepresentable, stream);
}

int mdct_jpegprog_dc_rows_approx(const mdct_jpegcoef_plane *planes, int n_planes, int interleaved, const mdct_jpegenc_opt_spec *specs, int ah, int al, size_t r0, size_t r1,
                                 uint8_t *out, size_t seg_stride, uint32_t *seg_bytes, uint32_t *ff_counts, uint32_t *uncoded, uint32_t *unrepresentable, void *stream)
{
  int rc, h, v;
  if ((rc = check_approx(ah, al)))
    return rc;
  if (!planes || (!specs && ah == 0) || !out || !seg_bytes || !ff_counts || !uncoded || !unrepresentable)
    return fail(MDCT_INVALID_PARAMETER, "null planes / specs / out / seg_bytes / ff_counts / uncoded / unrepresentable");
  uint32_t per_row, n_rows;
  if ((rc = check_dc_planes(planes, n_planes, interleaved, &h, &v, &per_row, &n_rows)))
    return rc;
  if (r0 >= r1 || r1 > n_rows)
    return fail(MDCT_INVALID_PARAMETER, "intervals [%zu, %zu) of %u", r0, r1, n_rows);
  const size_t blocks = (size_t)per_row * (size_t)(h ? h * v + 2 : 1);
  if ((rc = check_seg_stride(seg_stride, out, mdct_jpegenc_opt_seg_stride(blocks), 209, blocks, "interval", "the stride of the table-taking coders")))
    return rc;
  if ((rc = check_word(uncoded, "uncoded")) || (rc = check_word(unrepresentable, "unrepresentable")))
    return rc;
  DcArgs a;
  memset(&a, 0, sizeof(a));
  a.al = (uint32_t)al;
  a.refine = ah != 0; // raw bits, no table: nothing can be lost or lack a code
  bool complete = true;
  static const char *const names[2] = {"DC specification", "DC chrominance specification"};
  for (int w = 0; w < (h ? 2 : 1) && ah == 0; w++)
    if ((rc = spec_codes(&specs[w], false, names[w], a.dc[w], &complete)))
      return rc;
  a.complete = complete;
  dc_planes(a, planes, n_planes, per_row);
  a.out = out;
  a.seg_bytes = seg_bytes;
  a.ff_counts = ff_counts;
  a.uncoded = uncoded;
  a.unrepresentable = unrepresentable;
  a.seg_stride = seg_stride;
  a.my0 = (uint32_t)r0;
  return launch_dc<false>(a, h, v, (unsigned)(r1 - r0), (hipStream_t)stream);
}

int mdct_jpegprog_ac_stats(const mdct_jpegcoef_plane *plane, int ss, int se, uint32_t *hist, uint32_t *unrepresentable, void *stream)
{
  return mdct_jpegprog_ac_stats_approx(plane, ss, se, 0, 0, hist, unrepresentable, stream);
}

int mdct_jpegprog_ac_stats_approx(const mdct_jpegcoef_plane *plane, int ss, int se, int ah, int al, uint32_t *hist, uint32_t *unrepresentable, void *stream)
{
  if (!plane || !hist || !unrepresentable)
    return fail(MDCT_INVALID_PARAMETER, "null plane / hist / unrepresentable");
  int rc;
  if ((rc = check_word(hist, "hist")) || (rc = check_word(unrepresentable, "unrepresentable")) || (rc = check_coef_plane(*plane, "plane", 0)) || (rc = check_band(ss, se)) ||
      (rc = check_approx(ah, al)))
    return rc;
  BandArgs a;
  memset(&a, 0, sizeof(a));
  band_plane(a, *plane, ss, se);
  a.ah = (uint32_t)ah;
  a.al = (uint32_t)al;
  a.hist = hist;
  a.unrepresentable = unrepresentable;
  const hipStream_t s = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(hist, 0, sizeof(uint32_t) * 256, s);
  if (e != hipSuccess)
    return fail(MDCT_NOT_SUPPORTED, "memset: %s", hipGetErrorString(e));
  MDCT_LAUNCH((k_prog_ac<true>), dim3(plane->blocks_y), dim3(kBandThreads), 0, s, a);
  return launched();
}

int mdct_jpegprog_ac_rows(const mdct_jpegcoef_plane *plane, int ss, int se, size_t by0, size_t by1, const mdct_jpegenc_opt_spec *ac, uint8_t *out, size_t seg_stride,
                          uint32_t *seg_bytes, uint32_t *ff_counts, uint32_t *uncoded, uint32_t *unrepresentable, void *stream)
{
  return mdct_jpegprog_ac_rows_approx(plane, ss, se, 0, 0, by0, by1, ac, out, seg_stride, seg_bytes, ff_counts, uncoded, unrepresentable, stream);
}

int mdct_jpegprog_ac_rows_approx(const mdct_jpegcoef_plane *plane, int ss, int se, int ah, int al, size_t by0, size_t by1, const mdct_jpegenc_opt_spec *ac, uint8_t *out,
                                 size_t seg_stride, uint32_t *seg_bytes, uint32_t *ff_counts, uint32_t *uncoded, uint32_t *unrepresentable, void *stream)
{
  if (!plane || !out || !seg_bytes || !ff_counts || !uncoded || !unrepresentable)
    return fail(MDCT_INVALID_PARAMETER, "null plane / out / seg_bytes / ff_counts / uncoded / unrepresentable");
  int rc;
  if ((rc = check_coef_plane(*plane, "plane", 0)) || (rc = check_band(ss, se)) || (rc = check_approx(ah, al)))
    return rc;
  if (by0 >= by1 || by1 > plane->blocks_y)
    return fail(MDCT_INVALID_PARAMETER, "block rows [%zu, %zu) of %u", by0, by1, plane->blocks_y);
  if ((rc = check_seg_stride(seg_stride, out, mdct_jpegenc_opt_seg_stride(plane->blocks_x), 209, plane->blocks_x, "row", "1668 bits per block")))
    return rc;
  if ((rc = check_word(uncoded, "uncoded")) || (rc = check_word(unrepresentable, "unrepresentable")))
    return rc;
  BandArgs a;
  memset(&a, 0, sizeof(a));
  bool all = true;
  if ((rc = spec_codes(ac, true, "AC specification", a.ac, &all)))
    return rc;
  for (int n = 1; n < 15; n++) // and the EOBn of a band scan
    all = all && a.ac[n << 4];
  a.complete = all;
  band_plane(a, *plane, ss, se);
  a.ah = (uint32_t)ah;
  a.al = (uint32_t)al;
  a.out = out;
  a.seg_bytes = seg_bytes;
  a.ff_counts = ff_counts;
  a.uncoded = uncoded;
  a.unrepresentable = unrepresentable;
  a.seg_stride = seg_stride;
  a.by0 = (uint32_t)by0;
  MDCT_LAUNCH((k_prog_ac<false>), dim3((unsigned)(by1 - by0)), dim3(kBandThreads), 0, (hipStream_t)stream, a);
  return launched();
}

} // extern "C"
