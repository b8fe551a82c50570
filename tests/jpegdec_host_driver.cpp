// jpegdec_host_driver.cpp -- the host-compilable pieces of the JPEG decoders under sanitizers: huff_tables.h (build_tables with a real
// DevTables to write: every code of the tables it accepts decoded two ways, and the specifications it must refuse, between guard bytes)
// and block_place.h (the place of every block of five MCU layouts against ITU-T T.81 A.2.3 as written here, and the loop that zeroes a
// range of blocks).  Plain g++ with sanitizers (tests/test_jpeg_decode.py); nothing of the HIP runtime.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "block_place.h"
#include "huff_tables.h"

using namespace mdct::jpegdec;

namespace
{

int g_bad = 0;

#define EXPECT(cond, ...)                                                                                                                                     \
  do                                                                                                                                                          \
  {                                                                                                                                                           \
    if (!(cond))                                                                                                                                              \
    {                                                                                                                                                         \
      if (g_bad++ < 20)                                                                                                                                       \
      {                                                                                                                                                       \
        printf("FAIL %s: ", what);                                                                                                                            \
        printf(__VA_ARGS__);                                                                                                                                  \
        printf("\n");                                                                                                                                         \
      }                                                                                                                                                       \
    }                                                                                                                                                         \
  } while (0)

// ------------------------------------------------------------------------------------------------------------------ Huffman tables
struct Spec
{
  std::vector<uint8_t> bits, vals;
};

std::vector<uint8_t> from_hex(const char *h)
{
  std::vector<uint8_t> v;
  for (; h[0] && h[1]; h += 2)
  {
    unsigned x = 0;
    sscanf(h, "%2x", &x);
    v.push_back((uint8_t)x);
  }
  return v;
}

std::vector<uint8_t> iota(int n)
{
  std::vector<uint8_t> v;
  for (int i = 0; i < n; i++)
    v.push_back((uint8_t)i);
  return v;
}

// T.81 Annex K tables K.3 (DC luminance), K.4 (DC chrominance), K.5 (AC luminance), K.6 (AC chrominance)
const Spec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, iota(12)};
const Spec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, iota(12)};
const Spec kAcLuma = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
                      from_hex("01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
                               "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
                               "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")};
const Spec kAcChroma = {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
                        from_hex("000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
                                 "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4"
                                 "c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")};

// A DevTables between guard bytes, on the heap at its exact size (what is written past either end the sanitizers or the guards see).
// The far guard is longer than the farthest an over-subscribed specification made the unchecked loop write (255 codes of one bit:
// fast[t][.. 255 << 8], about 127 KiB past the struct).
struct Guarded
{
  static constexpr size_t kBefore = 4096, kAfter = 256 * 1024;
  uint8_t *mem;
  Guarded() : mem((uint8_t *)malloc(kBefore + sizeof(DevTables) + kAfter)) { memset(mem, 0xA5, kBefore + sizeof(DevTables) + kAfter); }
  ~Guarded() { free(mem); }
  DevTables *tables() { return (DevTables *)(mem + kBefore); }
  bool intact() const
  {
    for (size_t i = 0; i < kBefore; i++)
      if (mem[i] != 0xA5)
        return false;
    for (size_t i = 0; i < kAfter; i++)
      if (mem[kBefore + sizeof(DevTables) + i] != 0xA5)
        return false;
    return true;
  }
};
static_assert(Guarded::kBefore % alignof(DevTables) == 0, "the struct is aligned between its guards");

// build_tables on one specification in slot t (the other slots empty), with a real DevTables to write
int build_one(int t, const Spec &s, int nvals, DevTables *out)
{
  const uint8_t *bits[4] = {nullptr, nullptr, nullptr, nullptr}, *vals[4] = {nullptr, nullptr, nullptr, nullptr};
  int nv[4] = {0, 0, 0, 0};
  bool present[4];
  bits[t] = s.bits.data();
  vals[t] = s.vals.data();
  nv[t] = nvals;
  return build_tables(bits, vals, nv, out, present);
}

// huff() of jpegdec_common.h on the next 16 bits `peek` of the stream: the symbol and its code's length, -1 for no code
int lookup(const DevTables &T, int t, uint32_t peek, int *len)
{
  const uint32_t f = T.fast[t][peek >> (16 - kFastBits)];
  if (f)
  {
    *len = (int)(f >> 8);
    return (int)(f & 0xFF);
  }
  for (int l = kFastBits + 1; l <= 16; l++)
    if ((int32_t)peek < T.limit[t][l])
    {
      *len = l;
      return T.vals[t][((peek >> (16 - l)) + T.delta[t][l]) & 0xFF];
    }
  return -1;
}

// T.81 F.2.2.3 (figure F.16), one bit at a time, on tables of its own (C.2: mincode, maxcode, valptr)
int decode_bitwise(const Spec &s, uint32_t peek, int *len)
{
  int code = 0, first = 0, index = 0; // code read so far; the first code of this length; its value's index
  for (int l = 1; l <= 16; l++)
  {
    code = (code << 1) | (int)((peek >> (16 - l)) & 1);
    const int n = s.bits[l - 1];
    if (code - first < n)
    {
      *len = l;
      return s.vals[index + code - first];
    }
    index += n;
    first = (first + n) << 1;
  }
  return -1;
}

void accept(const char *what, int t, const Spec &s)
{
  Guarded gd;
  DevTables *T = gd.tables();
  const int rc = build_one(t, s, (int)s.vals.size(), T);
  EXPECT(rc == MDCT_SUCCESS, "refused with %d: %s", rc, g_err);
  EXPECT(gd.intact(), "wrote outside the DevTables");
  if (rc)
    return;
  // every code (C.2: codes of a length count up, a longer length starts at twice the next), followed by 0-bits and by 1-bits
  int code = 0, p = 0;
  for (int l = 1; l <= 16; l++)
  {
    for (int i = 0; i < s.bits[l - 1]; i++, code++, p++)
      for (int fill = 0; fill < 2; fill++)
      {
        const uint32_t peek = ((uint32_t)code << (16 - l)) | (fill ? (1u << (16 - l)) - 1u : 0u);
        int la = 0, lb = 0;
        const int a = lookup(*T, t, peek, &la), b = decode_bitwise(s, peek, &lb);
        EXPECT(b == s.vals[p] && lb == l, "the bit-by-bit decode of code %d of length %d gives symbol %d, length %d", code, l, b, lb);
        EXPECT(a == b && la == lb, "code %d of length %d: the table lookup gives symbol %d, length %d; bit by bit %d, %d", code, l, a, la, b, lb);
      }
    code <<= 1;
  }
  // and every 16-bit pattern at all: the same symbol and length, or no code in both
  for (uint32_t peek = 0; peek < 65536; peek++)
  {
    int la = 0, lb = 0;
    const int a = lookup(*T, t, peek, &la), b = decode_bitwise(s, peek, &lb);
    EXPECT(a == b && (a < 0 || la == lb), "pattern 0x%04x: the table lookup gives %d (%d bits), bit by bit %d (%d bits)", peek, a, la, b, lb);
  }
  printf("%s: %zu codes\n", what, s.vals.size());
}

void refuse(const char *what, int t, const Spec &s, int nvals, const char *message)
{
  Guarded gd;
  g_err[0] = 0;
  const int rc = build_one(t, s, nvals, gd.tables());
  EXPECT(rc == MDCT_INVALID_PARAMETER, "returned %d, not MDCT_INVALID_PARAMETER", rc);
  EXPECT(strcmp(g_err, message) == 0, "message \"%s\", expected \"%s\"", g_err, message);
  EXPECT(gd.intact(), "wrote outside the DevTables");
  printf("%s: %s\n", what, g_err);
}

Spec counts(int length, int n, uint8_t value)
{
  Spec s;
  s.bits.assign(16, 0);
  s.bits[length - 1] = (uint8_t)n;
  s.vals.assign((size_t)n, value);
  return s;
}

void huffman_tables()
{
  accept("K.3 DC luminance", 0, kDcLuma);
  accept("K.4 DC chrominance", 1, kDcChroma);
  accept("K.5 AC luminance", 2, kAcLuma);
  accept("K.6 AC chrominance", 3, kAcChroma);
  accept("one 16-bit code", 0, counts(16, 1, 5));

  refuse("three 1-bit codes", 0, counts(1, 3, 0), 3, "slot 0: codes over-subscribed at length 1");
  refuse("255 1-bit codes", 2, counts(1, 255, 0x01), 255, "slot 2: codes over-subscribed at length 1");
  refuse("five 2-bit codes", 1, counts(2, 5, 0), 5, "slot 1: codes over-subscribed at length 2");
  Spec ones = counts(2, 2, 0); // 0, 10, 11
  ones.bits[0] = 1;
  ones.vals.push_back(1);
  refuse("an all-ones code", 3, ones, 3, "slot 3: codes over-subscribed at length 2");
  Spec many = counts(8, 255, 0); // the counts are bytes: 257 values cannot agree with them, and are refused before they are compared
  many.vals.assign(257, 0);
  refuse("257 values", 2, many, 257, "slot 2: 257 values (at most 256)");
  refuse("counts that disagree with the values", 0, counts(2, 2, 0), 3, "slot 0: the 16 counts add up to 2 codes, 3 values given");
  refuse("DC category 12", 0, counts(4, 1, 12), 1, "slot 0: value 0x0c is not a baseline DC symbol");
  refuse("AC size 11", 2, counts(4, 1, 0x0B), 1, "slot 2: value 0x0b is not a baseline AC symbol");
}

// ------------------------------------------------------------------------------------------------------------------ block placement
struct Sampling
{
  const char *name;
  int n, h[3], v[3];
};

const Sampling kLayouts[] = {{"1x1 grey", 1, {1}, {1}},
                             {"4:4:4", 3, {1, 1, 1}, {1, 1, 1}},
                             {"4:2:2", 3, {2, 1, 1}, {1, 1, 1}},
                             {"4:4:0", 3, {1, 1, 1}, {2, 1, 1}},
                             {"4:2:0", 3, {2, 1, 1}, {2, 1, 1}}};
constexpr uint32_t kMcusX = 3, kMcusY = 2;

// the planes of one layout on the 3 x 2 MCU grid, rows 8 elements longer than the blocks need, each allocated at its exact size
struct Planes
{
  mdct_jpegdec_scan desc;
  size_t elems[3];
  Planes(const Sampling &s)
  {
    memset(&desc, 0, sizeof(desc));
    desc.n_components = s.n;
    desc.mcus_x = kMcusX;
    desc.mcus_y = kMcusY;
    for (int c = 0; c < s.n; c++)
    {
      mdct_jpegdec_component &q = desc.comp[c];
      q.h = s.h[c];
      q.v = s.v[c];
      q.blocks_x = kMcusX * (size_t)s.h[c];
      q.blocks_y = kMcusY * (size_t)s.v[c];
      q.pitch = q.blocks_x * 8 + 8;
      elems[c] = q.pitch * q.blocks_y * 8;
      q.coef = (int16_t *)aligned_alloc(16, elems[c] * sizeof(int16_t));
      q.dc_slot = 0;
      q.ac_slot = 2;
    }
  }
  ~Planes()
  {
    for (int c = 0; c < desc.n_components; c++)
      free(desc.comp[c].coef);
  }
  void fill()
  {
    for (int c = 0; c < desc.n_components; c++)
      for (size_t i = 0; i < elems[c]; i++)
        desc.comp[c].coef[i] = (int16_t)(1 + (i * 7 + (size_t)c * 13) % 1000);
  }
};

struct Block
{
  int comp;
  uint32_t row, col; // block row and column in the component's plane
};

// T.81 A.2.3: MCU after MCU, row by row over the MCU grid; inside an MCU component after component; inside a component its h x v
// blocks in rows of h, top to bottom.  MCU (mx, my) holds of that component the block rows my * v .. and the block columns mx * h ..
std::vector<Block> scan_order_a23(const Sampling &s)
{
  std::vector<Block> seq;
  for (uint32_t my = 0; my < kMcusY; my++)
    for (uint32_t mx = 0; mx < kMcusX; mx++)
      for (int c = 0; c < s.n; c++)
        for (uint32_t y = 0; y < (uint32_t)s.v[c]; y++)
          for (uint32_t x = 0; x < (uint32_t)s.h[c]; x++)
            seq.push_back(Block{c, my * s.v[c] + y, mx * s.h[c] + x});
  return seq;
}

// the layout as fill_geometry (jpegdec_common.h) hands it to the kernels
BlockPlace place_of(const mdct_jpegdec_scan &d)
{
  BlockPlace g;
  memset(&g, 0, sizeof(g));
  for (int c = 0; c < d.n_components; c++)
  {
    g.plane[c] = d.comp[c].coef;
    g.pitch[c] = d.comp[c].pitch;
    g.ch[c] = (uint32_t)d.comp[c].h;
    g.cv[c] = (uint32_t)d.comp[c].v;
    for (int v = 0; v < d.comp[c].v; v++)
      for (int h = 0; h < d.comp[c].h; h++, g.upm++)
      {
        g.bcomp[g.upm] = (uint8_t)c;
        g.bh[g.upm] = (uint8_t)h;
        g.bv[g.upm] = (uint8_t)v;
      }
  }
  g.mcus_x = (uint32_t)d.mcus_x;
  return g;
}

void placement(const Sampling &s)
{
  const char *what = s.name;
  Planes pl(s);
  const BlockPlace g = place_of(pl.desc);
  const std::vector<Block> seq = scan_order_a23(s);
  EXPECT(seq.size() == (size_t)kMcusX * kMcusY * g.upm, "A.2.3 gives %zu blocks, the layout %u per MCU", seq.size(), g.upm);
  std::vector<std::vector<int>> hits(3);
  for (int c = 0; c < s.n; c++)
    hits[c].assign(pl.desc.comp[c].blocks_x * pl.desc.comp[c].blocks_y, 0);
  for (uint32_t unit = 0; unit < seq.size(); unit++)
  {
    const Block &w = seq[unit];
    const struct
    {
      uint32_t mcu, b;
    } u = {unit / g.upm, unit % g.upm};
    const int c = g.bcomp[u.b];
    const uint32_t my = u.mcu / kMcusX, mx = u.mcu % kMcusX;
    const uint32_t row = my * g.cv[c] + g.bv[u.b], col = mx * g.ch[c] + g.bh[u.b];
    EXPECT(c == w.comp && row == w.row && col == w.col, "unit %u: (component %d, block row %u, column %u), A.2.3 says (%d, %u, %u)", unit, c, row, col,
           w.comp, w.row, w.col);
    const ptrdiff_t at = block_at(g, mx, my, u.b, (uint32_t)c, 0) - pl.desc.comp[w.comp].coef;
    const ptrdiff_t want = (ptrdiff_t)((size_t)w.row * 8 * pl.desc.comp[w.comp].pitch + (size_t)w.col * 8);
    EXPECT(at == want, "unit %u: element %td of its plane, A.2.3 says %td", unit, at, want);
    EXPECT(block_at(g, mx, my, u.b, (uint32_t)c, 5) == block_at(g, mx, my, u.b, (uint32_t)c, 0) + 5 * g.pitch[c], "unit %u: row 5 of the block", unit);
    if (w.row < pl.desc.comp[w.comp].blocks_y && w.col < pl.desc.comp[w.comp].blocks_x)
      hits[w.comp][w.row * pl.desc.comp[w.comp].blocks_x + w.col]++;
  }
  for (int c = 0; c < s.n; c++)
    for (size_t i = 0; i < hits[c].size(); i++)
      EXPECT(hits[c][i] == 1, "block %zu of component %d is hit %d times", i, c, hits[c][i]);
  printf("%s: %zu blocks placed\n", what, seq.size());
}

// zero_units over [z0, z0 + nz) of the interval at mcu0, every lane of a launch of `stride` lanes in turn: exactly those blocks go to zero
template <class I>
void zeroed(const Sampling &s, uint32_t mcu0, uint32_t z0, uint32_t nz, uint32_t stride)
{
  const std::string name = std::string(s.name) + ": zero_units(mcu0 " + std::to_string(mcu0) + ", z0 " + std::to_string(z0) + ", nz " + std::to_string(nz) +
                           ", stride " + std::to_string(stride) + ", " + std::to_string(sizeof(I) * 8) + "-bit)";
  const char *what = name.c_str();
  Planes pl(s), want(s);
  pl.fill();
  want.fill();
  const BlockPlace g = place_of(pl.desc);
  const std::vector<Block> seq = scan_order_a23(s);
  for (uint32_t unit = mcu0 * g.upm + z0; unit < mcu0 * g.upm + z0 + nz; unit++)
    for (int r = 0; r < 8; r++)
      memset(want.desc.comp[seq[unit].comp].coef + ((size_t)seq[unit].row * 8 + r) * want.desc.comp[seq[unit].comp].pitch + (size_t)seq[unit].col * 8, 0, 16);
  for (uint32_t lane = 0; lane < stride; lane++)
    zero_units<I>(g, mcu0, z0, nz, (I)lane, (I)stride);
  for (int c = 0; c < s.n; c++)
    for (size_t i = 0; i < pl.elems[c]; i++)
      if (pl.desc.comp[c].coef[i] != want.desc.comp[c].coef[i])
      {
        EXPECT(false, "component %d, element %zu (row %zu, column %zu) is %d, expected %d", c, i, i / pl.desc.comp[c].pitch, i % pl.desc.comp[c].pitch,
               pl.desc.comp[c].coef[i], want.desc.comp[c].coef[i]);
        break;
      }
}

void block_places()
{
  for (const Sampling &s : kLayouts)
  {
    placement(s);
    const uint32_t upm = [&] {
      uint32_t n = 0;
      for (int c = 0; c < s.n; c++)
        n += (uint32_t)(s.h[c] * s.v[c]);
      return n;
    }();
    const uint32_t units = kMcusX * kMcusY * upm;
    for (uint32_t stride : {256u, 1024u})
    {
      zeroed<uint32_t>(s, 0, 0, 0, stride);                             // nothing
      zeroed<uint64_t>(s, 0, 0, units, stride);                         // every unit
      zeroed<uint32_t>(s, 0, 0, units, stride);
      zeroed<uint32_t>(s, 0, upm + upm / 2, upm + 1, stride);           // from the middle of MCU 1 into MCU 2
      zeroed<uint64_t>(s, 0, units - upm - upm / 2 - 1, upm + upm / 2 + 1, stride); // ... of an MCU to the last unit
      zeroed<uint32_t>(s, 0, units - 1, 1, stride);                     // the last unit alone
      zeroed<uint32_t>(s, 0, units, 0, stride);                         // nothing, behind the last unit
      zeroed<uint64_t>(s, 2, upm / 2, 2 * upm, stride);                 // an interval that starts at MCU 2, across the MCU row's end
      zeroed<uint32_t>(s, 4, 1, 2 * upm - 1, stride);                   // ... at MCU 4, to the last unit
    }
    printf("%s: zero_units\n", s.name);
  }
}

} // namespace

int main()
{
  huffman_tables();
  block_places();
  if (g_bad)
  {
    printf("%d failures\n", g_bad);
    return 1;
  }
  printf("jpegdec host ok\n");
  return 0;
}
