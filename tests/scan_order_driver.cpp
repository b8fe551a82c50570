// scan_order_driver.cpp -- walks seq_block<H, V>(s) of scan_order.h, the permutation between the transform layout of a chunk and the
// scan order that k_scan_rows and k_opt code it in, for every thread of the four layouts, and holds it against a statement of
// ITU-T T.81 A.2.3 written here.  Plain g++ with sanitizers (tests/test_jpeg_encode_interleaved.py); nothing of the HIP runtime.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "scan_order.h"

using namespace mdct::scan_order;

namespace
{

struct Block
{
  int comp;     // 0 Y, 1 Cb, 2 Cr
  uint32_t row; // block row inside the MCU row
  uint32_t col; // block column, counted from the chunk's first MCU
  bool operator==(const Block &o) const { return comp == o.comp && row == o.row && col == o.col; }
};

int g_bad = 0;

#define EXPECT(cond, ...)                                                                                                                                     \
  do                                                                                                                                                          \
  {                                                                                                                                                           \
    if (!(cond))                                                                                                                                              \
    {                                                                                                                                                         \
      if (g_bad++ < 20)                                                                                                                                       \
      {                                                                                                                                                       \
        printf("FAIL <%d, %d> s = %u: ", H, V, s);                                                                                                            \
        printf(__VA_ARGS__);                                                                                                                                  \
        printf("\n");                                                                                                                                         \
      }                                                                                                                                                       \
    }                                                                                                                                                         \
  } while (0)

// The transform layout (scan_order.h's header, ScanChunks::init): the block that slot = wave * 64 + lane transforms.
template <int H, int V>
Block layout(uint32_t slot)
{
  const uint32_t wave = slot / 64, lane = slot % 64;
  if (H == 0) // one plane: 4 waves on 256 consecutive blocks
    return Block{0, 0, slot};
  if (H == 1) // 4:4:4: a wave per component, 64 consecutive blocks
    return Block{(int)wave, 0, lane};
  if (wave < (uint32_t)V) // a wave per luma block row, 64 consecutive blocks = 32 MCUs
    return Block{0, wave, lane};
  return Block{1 + (int)(lane / 32), 0, lane % 32}; // the chroma wave: Cb in lanes 0..31, Cr in lanes 32..63
}

// T.81 A.2.3: MCU after MCU; inside an MCU component after component; inside a component its h x v blocks row by row, left to right.
// MCU i of the chunk holds, of a component sampled h x v, the block rows 0..v-1 of the MCU row and the block columns i * h .. i * h + h - 1.
template <int H, int V>
std::vector<Block> scan_order_a23(uint32_t mcus, std::vector<uint32_t> *mcu_of)
{
  const int ncomp = H == 0 ? 1 : 3;
  std::vector<Block> seq;
  for (uint32_t i = 0; i < mcus; i++)
    for (int c = 0; c < ncomp; c++)
    {
      const uint32_t h = (H == 0 || c > 0) ? 1 : H, v = (H == 0 || c > 0) ? 1 : V;
      for (uint32_t y = 0; y < v; y++)
        for (uint32_t x = 0; x < h; x++)
        {
          seq.push_back(Block{c, y, i * h + x});
          mcu_of->push_back(i);
        }
    }
  return seq;
}

template <int H, int V>
void check()
{
  constexpr uint32_t T = 64 * kWaves<H, V>, M = kMcus<H, V>;
  static_assert(T == M * kBlocksPerMcu<H, V>, "one thread per block of the chunk");
  std::vector<uint32_t> mcu_of;
  const std::vector<Block> seq = scan_order_a23<H, V>(M, &mcu_of);
  uint32_t s = 0;
  EXPECT(seq.size() == T, "A.2.3 gives %zu blocks per chunk, the layout has %u threads", seq.size(), T);
  if (seq.size() != T)
    return;
  // slot_of[s]: the slot whose lane transformed the s-th block in scan order
  std::vector<uint32_t> slot_of(T, T);
  for (s = 0; s < T; s++)
    for (uint32_t slot = 0; slot < T; slot++)
      if (layout<H, V>(slot) == seq[s])
      {
        EXPECT(slot_of[s] == T, "the layout holds the block twice (slots %u and %u)", slot_of[s], slot);
        slot_of[s] = slot;
      }
  // per component: its last block of a chunk in scan order
  int last_of[3] = {-1, -1, -1};
  for (s = 0; s < T; s++)
    last_of[seq[s].comp] = (int)s;
  std::vector<int> hits(T, 0);
  int prev_of[3] = {-1, -1, -1}; // the component's previous block of this chunk in scan order
  for (s = 0; s < T; s++)
  {
    const SeqBlock b = seq_block<H, V>(s);
    const int c = seq[s].comp;
    EXPECT(slot_of[s] < T, "no slot transforms block (%d, %u, %u)", c, seq[s].row, seq[s].col);
    EXPECT(b.slot < T, "slot %u is outside [0, %u)", b.slot, T);
    if (b.slot < T)
      hits[b.slot]++;
    EXPECT(b.slot == slot_of[s], "slot %u, A.2.3 puts block (%d, %u, %u) = slot %u here", b.slot, c, seq[s].row, seq[s].col, slot_of[s]);
    EXPECT(b.mcu == mcu_of[s], "mcu %u, A.2.3 says %u", b.mcu, mcu_of[s]);
    EXPECT(b.chroma == (c > 0), "chroma %d for component %d", (int)b.chroma, c);
    EXPECT(b.pred < T, "pred %u is outside [0, %u)", b.pred, T);
    if (prev_of[c] < 0)
    { // the component's first block of the chunk: its predecessor is the component's last block of the chunk before
      EXPECT(b.carry, "carry is not set on component %d's first block of the chunk", c);
      EXPECT(b.pred == slot_of[last_of[c]], "pred %u, component %d's last block of a chunk is in slot %u", b.pred, c, slot_of[last_of[c]]);
    }
    else
    {
      EXPECT(!b.carry, "carry is set, but component %d has block %d of this chunk before it", c, prev_of[c]);
      EXPECT(b.pred == slot_of[prev_of[c]], "pred %u, the previous block of component %d is in slot %u", b.pred, c, slot_of[prev_of[c]]);
    }
    prev_of[c] = (int)s;
  }
  for (s = 0; s < T; s++)
    EXPECT(hits[s] == 1, "slot %u is coded by %d threads", s, hits[s]);
  printf("<%d, %d>: %u threads, %u MCUs per chunk\n", H, V, T, M);
}

} // namespace

int main()
{
  check<0, 0>();
  check<1, 1>();
  check<2, 1>();
  check<2, 2>();
  if (g_bad)
  {
    printf("%d failures\n", g_bad);
    return 1;
  }
  printf("scan order ok\n");
  return 0;
}
