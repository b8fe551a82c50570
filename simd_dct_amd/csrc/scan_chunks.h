// scan_chunks.h -- the chunk skeleton of the JPEG scan coders: k_scan_rows (jpeg_encode_scan.hip), k_opt (jpeg_encode_opt.hip) and
// k_coef (jpeg_coef.hip) work an MCU row (<0, 0>: a block row of one plane) through in chunks of kMcus MCUs = 64 * kWaves blocks, a
// chunk in two phases separated by a barrier (layouts and scan order: scan_order.h) --
//   transform  lane = block, COMPONENT-UNIFORM waves, so the quantiser multipliers stay wave-uniform scalar operands read from the
//              argument segment (two OwnTables, the wave picks one) and a wave's row loads are contiguous in one plane row.  Each lane
//              leaves its block's AC entries in its LDS row and (DC, entry count, EOB flag) in meta[].  The next chunk's pixel rows
//              are loaded before the barrier, in flight while this chunk is coded.  Lanes past the row's end redo the row's last block
//              and are not live.
//   symbols    thread s takes the s-th block of the chunk in scan order and reads the LDS row of the lane that transformed it; its
//              DC predictor is the previous block of the same component: a plain LDS read (meta[] of this chunk, or of the previous
//              chunk for the first block of a component -- meta is double-buffered --, or 0 at the row's start).
// ChunkGrid holds what does not depend on where the levels come from: which block a lane takes and the read-out of a block.  The
// source is a class on top of it: ScanChunks here (pixels -> AAN -> quantiser), CoefChunks (coef_chunks.h: a fetch from a
// coefficient plane).  The symbols phase and the epilogue are the kernels' (k_scan_rows its own, k_opt and k_coef: opt_symbols.h).
// Device code only.
#pragma once
#include "aan_passes.h"
#include "huffman_rows.h"
#include "own_tables.h"
#include "scan_order.h"

#pragma clang fp contract(off)

namespace mdct
{

// what the symbols phase needs of a block: AC entries in its LDS row, inside the row (a block past the row's end is coded by no
// one), DC level, DC predictor, whether an EOB follows the entries
struct ChunkBlock
{
  int n;
  bool live;
  int dc, pred;
  bool eob;
};

// Args: the kernel's argument struct.  The kernel's own type, not a common base: a source may read its tables at offsetof(Args, ...)
// of the argument segment.  The row's length in MCUs is Args' mcus_x where a launch codes one image; OwnRow: a kernel whose workgroups
// code rows of different images (k_batch_scan_rows, jpeg_encode_batch.hip) gives each workgroup its own, and Args has none.
template <int H, int V, class Args, bool OwnRow = false>
struct ChunkGrid
{
  static constexpr uint32_t kThreads = 64 * scan_order::kWaves<H, V>, M = scan_order::kMcus<H, V>;
  static_assert(kThreads == M * scan_order::kBlocksPerMcu<H, V>, "one symbols thread per block of the chunk");

  const Args &a;
  uint32_t own_mcus_x; // OwnRow only
  uint32_t tid, bx0, step, last_blk;
  uint16_t *rec;              // this lane's LDS row
  uint32_t (*meta)[kThreads]; // DC (low 16 bits) | entries << 16 | EOB needed << 24, by slot; [chunk parity]

  __device__ __forceinline__ explicit ChunkGrid(const Args &a_) : a(a_) { static_assert(!OwnRow, "an OwnRow grid is given its row's length"); }
  __device__ __forceinline__ ChunkGrid(const Args &a_, uint32_t mcus_x_) : a(a_), own_mcus_x(mcus_x_) { static_assert(OwnRow, "Args' mcus_x is the row's length"); }

  // MCUs in the row this workgroup codes
  __device__ __forceinline__ uint32_t row_mcus() const
  {
    if constexpr (OwnRow)
      return own_mcus_x;
    else
      return a.mcus_x;
  }

  // the transform phase's block of this thread: component, block row of its plane, first block and blocks per chunk
  __device__ __forceinline__ void place(uint32_t tid_, uint32_t lane, uint32_t wave, uint32_t my, uint16_t *rec_all, uint32_t (*meta_)[kThreads], uint32_t &comp,
                                        uint32_t &brow, bool &chroma_wave)
  {
    tid = tid_;
    meta = meta_;
    chroma_wave = H == 0 ? false : H == 1 ? wave > 0 : wave == (uint32_t)V;
    if (H == 0)
    {
      comp = 0;
      bx0 = tid;
      step = 256;
      last_blk = row_mcus() - 1;
      brow = my;
    }
    else if (H == 1)
    {
      comp = wave;
      bx0 = lane;
      step = 64;
      last_blk = row_mcus() - 1;
      brow = my;
    }
    else if (!chroma_wave)
    {
      comp = 0;
      bx0 = lane;
      step = 64;
      last_blk = 2 * row_mcus() - 1;
      brow = my * V + wave;
    }
    else
    {
      comp = 1 + (lane >> 5);
      bx0 = lane & 31;
      step = 32;
      last_blk = row_mcus() - 1;
      brow = my;
    }
    rec = rec_all + tid * kRec16Row;
  }

  // the lane's entries and (DC, entry count, EOB flag) of this chunk, from its 64 levels (low 16 bits of val[], natural order)
  __device__ __forceinline__ void leave(const uint32_t (&val)[64], uint32_t par)
  {
    int my_dc;
    bool need_eob;
    const uint32_t n = compact_levels16(val, rec, my_dc, need_eob);
    meta[par][tid] = ((uint32_t)my_dc & 0xFFFFu) | n << 16 | (need_eob ? 1u << 24 : 0u);
  }

  // after the barrier: the block sb of the chunk at MCU m0, read out of meta
  __device__ __forceinline__ ChunkBlock block(const scan_order::SeqBlock sb, uint32_t m0, uint32_t par) const
  {
    const uint32_t me = meta[par][sb.slot];
    ChunkBlock b;
    b.n = (int)((me >> 16) & 0xFFu);
    b.live = m0 + sb.mcu < row_mcus();
    b.dc = (int)(int16_t)(me & 0xFFFFu);
    b.pred = sb.carry ? (m0 == 0 ? 0 : (int)(int16_t)(meta[par ^ 1][sb.pred] & 0xFFFFu)) : (int)(int16_t)(meta[par][sb.pred] & 0xFFFFu);
    b.eob = (me >> 24) != 0;
    return b;
  }
};

// The pixel source.  Args: with tb[2], consts and dc_shift, and px[3], pitch[3], mcus_x where a launch codes one image (ScanArgs,
// OptArgs); the multiplier pairs are read at offsetof(Args, tb) of the argument segment.  A kernel whose workgroups code rows of
// different images (OwnRow) passes the row's length to the constructor and its image's planes to init.
template <int H, int V, class Args, bool OwnRow = false>
struct ScanChunks : ChunkGrid<H, V, Args, OwnRow>
{
  using Grid = ChunkGrid<H, V, Args, OwnRow>;
  using Grid::a;
  using Grid::bx0;
  using Grid::last_blk;
  using Grid::M;
  using Grid::step;
  static constexpr bool kCountsLoss = false; // the quantiser saturates: nothing to report

  size_t pitch;
  const uint8_t *src_row;
  uint2 rows[8];
  karg_pairs_t qf;

  __device__ __forceinline__ explicit ScanChunks(const Args &a_) : Grid(a_) {}
  __device__ __forceinline__ ScanChunks(const Args &a_, uint32_t mcus_x_) : Grid(a_, mcus_x_) {}

  // the 8 rows of block min(bx, last) of the block row (lanes past the row's end redo the last block)
  __device__ __forceinline__ void fetch(uint32_t bx)
  {
    const uint8_t *src = src_row + (size_t)min(bx, last_blk) * 8;
#pragma unroll
    for (int r = 0; r < 8; r++)
      rows[r] = load8(src + (size_t)r * pitch);
  }

  // the transform phase's block of this thread (ChunkGrid::place) in its plane; its first rows are requested
  __device__ __forceinline__ void init(uint32_t tid_, uint32_t lane, uint32_t wave, uint32_t my, uint16_t *rec_all, uint32_t (*meta_)[Grid::kThreads])
  {
    init(tid_, lane, wave, my, rec_all, meta_, a.px[0], a.px[1], a.px[2], a.pitch[0], a.pitch[1], a.pitch[2]);
  }

  // ... in the planes given (wave-uniform values)
  __device__ __forceinline__ void init(uint32_t tid_, uint32_t lane, uint32_t wave, uint32_t my, uint16_t *rec_all, uint32_t (*meta_)[Grid::kThreads],
                                       const uint8_t *px0, const uint8_t *px1, const uint8_t *px2, size_t pitch0, size_t pitch1, size_t pitch2)
  {
    uint32_t comp, brow;
    bool chroma_wave;
    Grid::place(tid_, lane, wave, my, rec_all, meta_, comp, brow, chroma_wave);
    // (selects, not an index: the argument block stays in scalar registers)
    pitch = comp == 0 ? pitch0 : comp == 1 ? pitch1 : pitch2;
    src_row = (comp == 0 ? px0 : comp == 1 ? px1 : px2) + (size_t)brow * 8 * pitch;
    fetch(bx0);
    // the multiplier pairs of this wave's table (wave-uniform: scalar loads from the argument segment)
    qf = karg_pairs(offsetof(Args, tb) + (chroma_wave ? sizeof(OwnTables) : 0) + offsetof(OwnTables, qf));
  }

  // chunk number `chunk`, at MCU m0 of the row: rows -> levels -> entries in the lane's LDS row and meta[par][tid]; then the next
  // chunk's rows are requested.  The caller's barrier follows.
  __device__ __forceinline__ void transform(uint32_t m0, uint32_t chunk, uint32_t par)
  {
    const AanPk &K = reinterpret_cast<const AanPk &>(a.consts);
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
    Grid::leave(val, par);
    if (m0 + M < Grid::row_mcus())
      fetch(bx0 + (chunk + 1) * step);
  }
};

} // namespace mdct
