// jpegdec_common.h -- what the JPEG decoder libraries share (jpeg_decode.hip: restart-marked scans, libmdct_jpegdec.so;
// jpeg_decode_unmarked.hip: scans without restart markers, libmdct_jpegdec_unmarked.so; jpeg_decode_batch.hip: the restart-marked scans
// of many files in one grid, libmdct_jpegdec_batch.so, which runs decode_interval and the index passes below as jpeg_decode.hip
// does; jpeg_decode_progressive.hip: the scans of a progressive file, libmdct_jpegdec_prog.so): the device Huffman tables and the handle
// that owns them (huff_tables.h), the block layout (block_place.h), the bit reader with its unstuffing, the Huffman lookup, the scan
// grammars (Sequential: baseline; Band<AC>: a progressive first scan), the one sub-sequence decoder `run` over them, the skeleton every
// decoder hangs it in -- a lane's sub-sequence (SubLane), the speculative first pass, the settle loop that synchronises the lanes of a
// workgroup, the write pass -- an interval's bookkeeping (interval_of, put_status), the prefix sums and the host's descriptor checks.
// Each library includes it from exactly one translation unit; everything here has internal linkage or is a device function.
#pragma once
#include <hip/hip_runtime.h>

#include "block_place.h" // mdct_jpegdec.h
#include "huff_tables.h" // host_error.h, mdct.h
#include "wg_sync.h"

// the message of this library's last failure (each library has its own)
namespace
{
int hip_fail(hipError_t e, const char *what) { return fail(MDCT_NOT_SUPPORTED, "%s: %s", what, hipGetErrorString(e)); }
} // namespace

namespace mdct
{
namespace jpegdec
{

constexpr int kThreads = 256;   // lanes per restart interval
constexpr uint32_t kErr = 0x80000000u;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr uint32_t kMaxCount = 0x7FFFFFFFu; // where a lane's block count saturates (a garbage EOBn adds up to 32767 per symbol)

struct DecArgs
{
  const uint8_t *scan;
  uint64_t scan_len;
  const uint64_t *off;
  uint32_t *status;
  const DevTables *tab;
  BlockPlace g;                 // where block b of MCU m lies
  uint8_t bdc[MDCT_JPEGDEC_MAX_BLOCKS_PER_MCU], bac[MDCT_JPEGDEC_MAX_BLOCKS_PER_MCU]; // table slots of block b
  uint32_t total_mcus, restart;
  uint32_t n_intervals;
};

static __constant__ uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ------------------------------------------------------------------------------------------------------------------ the bit reader
struct Reader
{
  const uint8_t *scan;
  uint64_t len;      // the whole scan: no byte outside [scan, scan + len) is read
  uint64_t p, end;   // next stuffed byte, end of the interval's data
  uint64_t E;        // first stuffed byte of the next sub-sequence (UINT64_MAX: none)
  uint64_t buf;      // left-aligned
  uint32_t nb;       // bits in buf
  uint32_t u;        // bits consumed since the lane's start (after unstuffing)
  uint32_t ufill;    // bits appended since the lane's start
  uint32_t uE;       // ufill when the first data byte at or after E was appended (kNone: not yet)
  uint32_t uend;     // ufill when the data ran out (kNone: not yet)
  bool dry, marker;
  uintptr_t wa;      // address of the cached aligned word
  uint32_t w;
};

__device__ __forceinline__ uint32_t byte_at(Reader &r, uint64_t p)
{
  const uintptr_t q = (uintptr_t)(r.scan + p);
  const uintptr_t a = q & ~uintptr_t(3);
  if (a != r.wa)
  {
    if (a < (uintptr_t)r.scan || a + 4 > (uintptr_t)(r.scan + r.len))
      return r.scan[p]; // a word that would leave the buffer: this byte alone
    r.w = *(const uint32_t *)a;
    r.wa = a;
  }
  return (r.w >> (8 * (q & 3))) & 0xFFu;
}

__device__ __forceinline__ void refill(Reader &r)
{
  while (r.nb <= 56) // at most 8 rounds
  {
    uint32_t b = 0;
    if (!r.dry)
    {
      if (r.p >= r.end)
      {
        r.dry = true;
        r.uend = r.ufill;
      }
      else
      {
        b = byte_at(r, r.p);
        uint32_t step = 1;
        if (b == 0xFF)
        {
          const uint32_t b2 = r.p + 1 < r.end ? byte_at(r, r.p + 1) : 0x100u;
          if (b2 == 0)
            step = 2;
          else
          {
            r.dry = r.marker = true;
            r.uend = r.ufill;
            b = 0;
          }
        }
        if (!r.dry)
        {
          if (r.uE == kNone && r.p >= r.E)
            r.uE = r.ufill;
          r.p += step;
        }
      }
    }
    r.buf |= (uint64_t)b << (56 - r.nb);
    r.nb += 8;
    r.ufill += 8;
  }
}

__device__ __forceinline__ void consume(Reader &r, uint32_t n)
{
  r.buf <<= n;
  r.nb -= n;
  r.u += n;
}

__device__ __forceinline__ uint32_t get_bits(Reader &r, uint32_t s)
{
  const uint32_t v = s ? (uint32_t)(r.buf >> (64 - s)) : 0u;
  consume(r, s);
  return v;
}

__device__ __forceinline__ int extend(uint32_t v, uint32_t s)
{
  return s == 0 ? 0 : ((int)v < (1 << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v);
}

__device__ __forceinline__ bool overrun(const Reader &r) { return r.dry && r.u > r.uend; }

__device__ __forceinline__ uint32_t data_error(const Reader &r) { return r.marker ? MDCT_JPEGDEC_UNEXPECTED_MARKER : MDCT_JPEGDEC_OUT_OF_DATA; }

// no code matched the next 16 bits: an invalid code if 16 bits of data were there, else the data ran out first
__device__ __forceinline__ uint32_t no_code(const Reader &r) { return r.dry && r.u + 16 > r.uend ? data_error(r) : MDCT_JPEGDEC_BAD_CODE; }

// one Huffman symbol of table t (LDS); returns -1 for a pattern that is no code
__device__ __forceinline__ int huff(Reader &r, const DevTables &T, int t)
{
  const uint32_t peek = (uint32_t)(r.buf >> 48);
  const uint32_t f = T.fast[t][peek >> (16 - kFastBits)];
  if (f)
  {
    consume(r, f >> 8);
    return (int)(f & 0xFF);
  }
  for (int l = kFastBits + 1; l <= 16; l++)
    if ((int32_t)peek < T.limit[t][l])
    {
      consume(r, l);
      return T.vals[t][((peek >> (16 - l)) + T.delta[t][l]) & 0xFF];
    }
  return -1;
}

struct Lane
{
  uint32_t state;    // packed start / exit state: kErr | d << 12 | k << 4 | b
  int blocks;        // blocks completed (a Band grammar: end-of-band runs included, saturating at kMaxCount)
  int dc[3];         // sum of the DC differences per component
  uint32_t err;      // MDCT_JPEGDEC_* of a decode error (final pass)
  bool finished;     // completed the interval's last block (final pass)
  uint32_t fin;      // status after the last block: OK / LEFTOVER / UNEXPECTED_MARKER
};

// ------------------------------------------------------------------------------------------------------------------ the scan grammars
// What `run` decodes.  Sequential: a baseline scan (T.81 F.2.2): per block the DC symbol at k == 0, then AC symbols up to position 63;
// S = 0 without ZRL ends the block.  Band<AC>: a first scan of a progressive file (G.1.2), levels in units of 1 << al: the DC scan
// (every symbol a DC symbol) or an AC band ss..se (no DC symbol; S = 0 without ZRL is EOBn, ending (1 << R) + (R extra bits) blocks).
enum class Scan { Sequential, DcFirst, AcBand };
struct Sequential
{
  static constexpr Scan kind = Scan::Sequential;
  static constexpr uint32_t ss = 0, se = 63, al = 0;
};

template <bool AC>
struct Band // an AC band: one block per MCU (the block in MCU stays 0), and EOBn runs
{
  static constexpr Scan kind = Scan::AcBand;
  uint32_t ss, se, al;
};
template <>
struct Band<false> // the DC scan: its band is 0..0 by definition
{
  static constexpr Scan kind = Scan::DcFirst;
  static constexpr uint32_t ss = 0, se = 0;
  uint32_t al;
  __device__ Band(uint32_t, uint32_t, uint32_t al_) : al(al_) {}
};

__device__ __forceinline__ void reader_init(Reader &r, const DecArgs &a, uint64_t s0, uint64_t end, uint64_t E, bool first)
{
  r.scan = a.scan;
  r.len = a.scan_len;
  r.p = s0;
  r.end = end;
  r.E = E;
  r.buf = 0;
  r.nb = 0;
  r.u = r.ufill = 0;
  r.uE = r.uend = kNone;
  r.dry = r.marker = false;
  r.wa = 1;
  r.w = 0;
  if (!first && s0 < end && s0 > 0 && byte_at(r, s0 - 1) == 0xFF)
  {
    if (byte_at(r, s0) == 0)
      r.p = s0 + 1; // s0 is the stuffed zero after a data 0xFF
    else
    {
      r.dry = r.marker = true; // s0 is inside a marker
      r.uend = 0;
    }
  }
}

// the interval's last block is complete: what follows must be its padding (1-bits to the byte boundary) and nothing else
__device__ __forceinline__ uint32_t after_last_block(Reader &r)
{
  refill(r);
  uint32_t fin = MDCT_JPEGDEC_LEFTOVER;
  if (r.dry)
  {
    const uint32_t rem = r.uend - r.u;
    if (rem < 8 && (rem == 0 || (uint32_t)(r.buf >> (64 - rem)) == (1u << rem) - 1u))
      fin = r.marker ? MDCT_JPEGDEC_UNEXPECTED_MARKER : MDCT_JPEGDEC_OK;
  }
  return fin;
}

// Decode from state `start` until the first symbol boundary at or after the next sub-sequence's start (a lane with a successor), the
// interval's last block (WRITE with a unit budget), or an error.  WRITE: unit0 blocks precede the start; pred = DC predictors there.
template <bool WRITE, class G>
__device__ void run(Reader &r, const DecArgs &a, const G &gr, const DevTables &T, const uint32_t *lcomp, uint32_t start, Lane &out,
                    uint32_t unit0, uint32_t units, uint32_t mcu0, int pred[3], uint64_t cap)
{
  constexpr bool kAcBand = G::kind == Scan::AcBand;
  out.blocks = 0;
  out.dc[0] = out.dc[1] = out.dc[2] = 0;
  out.err = 0;
  out.finished = false;
  out.fin = 0;
  out.state = kErr;
  if (start & kErr)
    return;
  uint32_t k = (start >> 4) & 0x7F, b = start & 0xF;
  uint32_t d = start >> 12;
  for (uint32_t i = 0; i < 64 && d > 0; i++) // skip the bits the previous lane consumed past this sub-sequence's start
  {
    refill(r);
    const uint32_t n = d < 32 ? d : 32;
    consume(r, n);
    d -= n;
  }
  if (overrun(r))
  {
    out.err = data_error(r);
    return;
  }
  uint32_t unit = unit0;
  if (WRITE && unit >= units)
    return;
  // the current block's place (WRITE): MCU (mx, my), block b of it
  uint32_t mx = 0, my = 0;
  int16_t *bp = nullptr;
  uint32_t comp = lcomp[b];
  if (WRITE)
  {
    const uint32_t mcu = mcu0 + unit / a.g.upm;
    my = mcu / a.g.mcus_x;
    mx = mcu - my * a.g.mcus_x;
    bp = block_at(a.g, mx, my, b, comp, 0);
  }
  for (uint64_t it = 0; it < cap; it++)
  {
    refill(r);
    if (r.uE != kNone && r.u >= r.uE)
    {
      out.state = ((r.u - r.uE) << 12) | (k << 4) | b;
      return;
    }
    bool block_end = false; // the symbol completes a block ...
    uint32_t ended = 1;     // ... and with it this many (an EOBn: the run)
    const bool dc = G::kind == Scan::DcFirst || (G::kind == Scan::Sequential && k == 0); // a DC symbol comes
    const int sym = huff(r, T, dc ? a.bdc[b] : a.bac[kAcBand ? 0 : b]);
    if (sym < 0)
    {
      out.err = no_code(r);
      if (WRITE || out.err != MDCT_JPEGDEC_BAD_CODE)
        return;
      consume(r, 1); // speculating: resynchronise instead of stopping (see the kernel's comment)
      out.err = 0;
      block_end = true;
    }
    else if (dc)
    {
      const uint32_t s = (uint32_t)sym & 15;
      const int diff = extend(get_bits(r, s), s);
      if (overrun(r))
      {
        out.err = data_error(r);
        return;
      }
      out.dc[comp] += diff;
      if (WRITE)
      {
        pred[comp] += diff;
        bp[0] = (int16_t)((uint32_t)pred[comp] << gr.al);
      }
      k = 1;
      block_end = gr.se == 0;
    }
    else
    {
      if (overrun(r))
      {
        out.err = data_error(r);
        return;
      }
      const uint32_t run_ = (uint32_t)sym >> 4, s = (uint32_t)sym & 15;
      if (s == 0)
      {
        if (run_ == 15) // ZRL
        {
          k += 16;
          if (k > gr.se + 1)
          {
            if (WRITE)
            {
              out.err = MDCT_JPEGDEC_COEF_OVERFLOW;
              return;
            }
            k = gr.se + 1; // speculating: end the block
          }
          block_end = k == gr.se + 1;
        }
        else // EOB, EOBn
        {
          block_end = true;
          if constexpr (kAcBand)
          {
            ended = (1u << run_) + get_bits(r, run_);
            if (overrun(r))
            {
              out.err = data_error(r);
              return;
            }
          }
        }
      }
      else
      {
        k += run_;
        if (k > gr.se)
        {
          if (WRITE)
          {
            out.err = MDCT_JPEGDEC_COEF_OVERFLOW;
            return;
          }
          k = gr.se; // speculating: keep the bit position, end the block after this level
        }
        const int v = extend(get_bits(r, s), s);
        if (overrun(r))
        {
          out.err = data_error(r);
          return;
        }
        if (WRITE)
        {
          const uint32_t z = kZigzag[k];
          bp[(size_t)(z >> 3) * a.g.pitch[comp] + (z & 7)] = (int16_t)((uint32_t)v << gr.al);
        }
        k++;
        block_end = k == gr.se + 1;
      }
    }
    if (block_end)
    {
      k = gr.ss;
      if constexpr (kAcBand)
      {
        if (WRITE && ended > units - unit) // unit < units here; the block of the EOBn is the failing one
        {
          out.err = MDCT_JPEGDEC_EOBRUN_OVERFLOW;
          return;
        }
        out.blocks = (int)((uint32_t)out.blocks + ended < kMaxCount ? (uint32_t)out.blocks + ended : kMaxCount);
      }
      else
        out.blocks++;
      if constexpr (!kAcBand)
      {
        if (++b == a.g.upm)
          b = 0;
        comp = lcomp[b];
      }
      if (WRITE)
      {
        unit += ended;
        if (unit == units)
        {
          out.finished = true;
          out.fin = after_last_block(r);
          return;
        }
        if (kAcBand && ended > 1) // a run is an AC band's, one block per MCU: over its blocks
        {
          const uint32_t mcu = mcu0 + unit;
          my = mcu / a.g.mcus_x;
          mx = mcu - my * a.g.mcus_x;
        }
        else if (b == 0 && ++mx == a.g.mcus_x)
        {
          mx = 0;
          my++;
        }
        bp = block_at(a.g, mx, my, b, comp, 0);
      }
    }
  }
  out.err = MDCT_JPEGDEC_OUT_OF_DATA; // not reached: every symbol consumes a bit and the data ends
}

__device__ __forceinline__ int wave_incl_scan(int x, int lane)
{
  for (int o = 1; o < 64; o <<= 1)
  {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o)
      x += y;
  }
  return x;
}

// exclusive prefix of x over a workgroup of any number of waves, 4 or 16 here (wtot: an int per wave, each wave adding those before its own)
__device__ __forceinline__ int wg_excl_scan(int x, int *wtot)
{
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int inc = wave_incl_scan(x, lane);
  if (lane == 63)
    wtot[w] = inc;
  wg_sync();
  int base = 0;
  for (int j = 0; j < w; j++)
    base += wtot[j];
  wg_sync();
  return base + inc - x;
}

// exclusive prefix of src[0 .. n) into dst (which may be src) over one workgroup of 1024 lanes (wtot: 16 ints); returns the total
template <class T>
__device__ T wg1024_excl_prefix(const T *src, T *dst, uint32_t n, int *wtot)
{
  const uint32_t per = (n + 1023) / 1024;
  const uint32_t c0 = threadIdx.x * per, c1 = c0 + per < n ? c0 + per : n;
  T sum = 0;
  for (uint32_t c = c0; c < c1; c++)
    sum += src[c];
  T run_ = (T)wg_excl_scan((int)sum, wtot);
  int total = 0;
  for (int j = 0; j < 16; j++)
    total += wtot[j];
  for (uint32_t c = c0; c < c1; c++)
  {
    const T m = src[c];
    dst[c] = run_;
    run_ += m;
  }
  wg_sync();
  return (T)total;
}

// ------------------------------------------------------------------------------------------------------------------ the skeleton
// A lane's sub-sequence: the bytes [s, end) are cut into sub-sequences of sb bytes, lane i of the workgroup on the i-th.  An interval
// (sb = max(8, ceil(n / kThreads)), end = its trimmed end) over one workgroup, or an unmarked scan's chunk (kSubBytes, end = the scan's).
struct SubLane
{
  uint64_t s0, end; // this lane's first byte, the end of the data
  uint64_t E;       // the next sub-sequence's first byte (UINT64_MAX: none)
  uint64_t cap;     // bound of the decode loop: every trip consumes a bit
  uint32_t nact;    // lanes of the workgroup with data (at least 1)
  bool active, first; // first: the lane's start is exact, not a guess (first0: lane 0's is)
};

__device__ __forceinline__ SubLane sub_lane(uint64_t s, uint64_t end, uint64_t sb, int tid, bool first0)
{
  SubLane q;
  const uint64_t n = end > s ? end - s : 0, lanes = (n + sb - 1) / sb;
  q.nact = n ? (uint32_t)(lanes < (uint64_t)kThreads ? lanes : (uint64_t)kThreads) : 1u;
  q.active = (uint32_t)tid < q.nact;
  q.s0 = s + (uint64_t)tid * sb;
  q.end = end;
  q.E = q.s0 + sb < end ? q.s0 + sb : ~uint64_t(0);
  q.cap = 8 * (end - (q.s0 < end ? q.s0 : end)) + 64;
  q.first = first0 && tid == 0;
  return q;
}

// the tables and the blocks' components into LDS (lcomp: 16 words) by a workgroup of `lanes` lanes; the caller synchronises
__device__ __forceinline__ void load_tables(const DecArgs &a, DevTables &T, uint32_t *lcomp, int tid, int lanes = kThreads)
{
  const uint32_t *src = (const uint32_t *)a.tab;
  uint32_t *dst = (uint32_t *)&T;
  for (int i = tid; i < (int)(sizeof(DevTables) / 4); i += lanes)
    dst[i] = src[i];
  if (tid < 16)
    lcomp[tid] = tid < (int)a.g.upm ? a.g.bcomp[tid] : 0;
}

// One speculating decode of the lane's sub-sequence from state `start`; a lane without data publishes no usable exit, no blocks, no DC.
// The first pass starts every lane from the same guess: bit 0 of its first byte, the first position (ss) of an MCU's first block.
template <class G>
__device__ __forceinline__ void speculate(const DecArgs &a, const G &gr, const DevTables &T, const uint32_t *lcomp, const SubLane &q,
                                          uint32_t start, Lane &L)
{
  Reader r;
  int dummy[3] = {0, 0, 0};
  L.state = kErr;
  L.blocks = L.dc[0] = L.dc[1] = L.dc[2] = 0;
  if (!q.active)
    return;
  reader_init(r, a, q.s0, q.end, q.E, q.first);
  run<false>(r, a, gr, T, lcomp, start, L, 0, 0, 0, dummy, q.cap);
}

// The synchronisation inside a workgroup: lane 0 wants want0, lane i the exit of lane i - 1; a lane whose start differs decodes again,
// until no start changes (at most nact + 1 trips: each trip makes one more lane exact).  exit_state: kThreads words of LDS, every
// lane's exit state on return.  Returns whether this lane decoded again.
template <class G>
__device__ __forceinline__ bool settle(const DecArgs &a, const G &gr, const DevTables &T, const uint32_t *lcomp, const SubLane &q,
                                       uint32_t want0, uint32_t &my_start, Lane &L, uint32_t *exit_state)
{
  bool ran = false;
  exit_state[threadIdx.x] = L.state;
  for (uint32_t round = 0; round <= q.nact; round++)
  {
    wg_sync();
    const uint32_t want = threadIdx.x == 0 ? want0 : exit_state[threadIdx.x - 1];
    const bool changed = q.active && want != my_start;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (!__syncthreads_or(changed))
      break;
    if (changed)
    {
      my_start = want;
      speculate(a, gr, T, lcomp, q, my_start, L);
      exit_state[threadIdx.x] = L.state;
      ran = true;
    }
  }
  wg_sync();
  return ran;
}

// The write pass of a lane with data: the exact decode from `start`, unit0 blocks and the predictors `pred` before it, writing levels.
// A decode error goes to *first_err (LDS, kNone before) as lane << 8 | code, the smallest winning; the status after the range's last
// block to *fin.  Returns the unit the lane stopped in (unit0 + the blocks it completed): the failing one in the lane that wins.
template <class G>
__device__ __forceinline__ uint32_t write_pass(const DecArgs &a, const G &gr, const DevTables &T, const uint32_t *lcomp, const SubLane &q,
                                               uint32_t start, uint32_t unit0, uint32_t units, uint32_t mcu0, int pred[3],
                                               uint32_t *first_err, uint32_t *fin)
{
  Reader r;
  Lane F;
  reader_init(r, a, q.s0, q.end, q.E, q.first);
  run<true>(r, a, gr, T, lcomp, start, F, unit0, units, mcu0, pred, q.cap);
  if (F.err && unit0 < units)
    atomicMin(first_err, ((uint32_t)threadIdx.x << 8) | F.err);
  if (F.finished)
    *fin = F.fin;
  return unit0 + (uint32_t)F.blocks;
}

// ------------------------------------------------------------------------------------------------------------------ one restart interval
// Interval k of the scan `a` describes, for the progressive scans (jpeg_decode_progressive.hip).  decode_interval below holds the same
// statements in line, and a change to one goes into the other: taken from here, k_decode was 1.5-2 % slower.
struct Interval
{
  uint64_t s, e, next;  // its data [s, e), clamped into the scan whatever the offsets say; off[k + 1] as given
  uint64_t sb;          // bytes per lane's sub-sequence when one workgroup of kThreads lanes decodes it
  bool last;
  uint32_t mcu0, units; // its first MCU, its blocks
};

__device__ __forceinline__ Interval interval_of(const DecArgs &a, const uint32_t k)
{
  Interval iv;
  const uint64_t len = a.scan_len;
  iv.last = k + 1 == a.n_intervals;
  uint64_t s = a.off[k];
  iv.next = a.off[k + 1];
  uint64_t e = iv.last ? iv.next : (iv.next >= 2 ? iv.next - 2 : 0);
  s = s < len ? s : len;
  e = e < len ? e : len;
  e = e > s ? e : s;
  // T.81 B.1.1.2: 0xFF bytes directly before the interval's RSTm are fill bytes, not data
  if (!iv.last && iv.next <= len)
    for (uint64_t i = 0, n = e - s; i < n && a.scan[e - 1] == 0xFF; i++)
      e--;
  iv.s = s;
  iv.e = e;
  const uint64_t sb = (e - s + kThreads - 1) / kThreads;
  iv.sb = sb < 8 ? 8 : sb;
  iv.mcu0 = k * a.restart;
  const uint32_t nmcu = (a.total_mcus - iv.mcu0) < a.restart ? a.total_mcus - iv.mcu0 : a.restart;
  iv.units = nmcu * a.g.upm;
  return iv;
}

// lane 0: the interval's status, once its data is judged: the marker after an interval that is not the last must be RST(k mod 8)
__device__ __forceinline__ void put_status(const DecArgs &a, const Interval &iv, const uint32_t k, uint32_t st)
{
  if (st == MDCT_JPEGDEC_OK && !iv.last)
  {
    const uint64_t next = iv.next;
    const bool ok = next >= 2 && next <= a.scan_len && next - 2 >= iv.s && a.scan[next - 2] == 0xFF && a.scan[next - 1] == 0xD0 + (k & 7);
    if (!ok)
      st = MDCT_JPEGDEC_UNEXPECTED_MARKER;
  }
  a.status[k] = st;
}

// The whole of k_decode (jpeg_decode.hip) for interval k, run by one workgroup of kThreads lanes; k_decode_batch (jpeg_decode_batch.hip)
// calls it with a scan record it looked up and the interval's index within that scan.
__device__ __forceinline__ void decode_interval(const DecArgs &a, const uint32_t k)
{
  __shared__ DevTables T;
  __shared__ uint32_t exit_state[kThreads];
  __shared__ uint32_t lcomp[16];
  __shared__ int wtot[kThreads / 64];
  __shared__ uint32_t first_err, fin_word, fail_unit;
  const int tid = threadIdx.x;
  const Sequential gr;
  load_tables(a, T, lcomp, tid);
  if (tid == 0)
  {
    first_err = kNone;
    fin_word = kNone;
  }
  // the interval's data, clamped into the scan whatever the offsets say
  const uint64_t len = a.scan_len;
  const bool last = k + 1 == a.n_intervals;
  uint64_t s = a.off[k];
  const uint64_t next = a.off[k + 1];
  uint64_t e = last ? next : (next >= 2 ? next - 2 : 0);
  s = s < len ? s : len;
  e = e < len ? e : len;
  e = e > s ? e : s;
  // T.81 B.1.1.2: 0xFF bytes directly before the interval's RSTm are fill bytes, not data (a data 0xFF is always followed by its
  // stuffed zero).  The last interval's end is the scan's, which the caller gives without them.
  if (!last && next <= len)
    for (uint64_t i = 0, n = e - s; i < n && a.scan[e - 1] == 0xFF; i++)
      e--;
  const uint64_t sb = (e - s + kThreads - 1) / kThreads;
  const SubLane q = sub_lane(s, e, sb < 8 ? 8 : sb, tid, true);
  const uint32_t mcu0 = k * a.restart;
  const uint32_t nmcu = (a.total_mcus - mcu0) < a.restart ? a.total_mcus - mcu0 : a.restart;
  const uint32_t units = nmcu * a.g.upm;
  wg_sync();

  // ---- synchronisation: lane 0 starts exact, the others from a guess, until no start changes
  Lane L;
  uint32_t my_start = 0;
  speculate(a, gr, T, lcomp, q, my_start, L);
  settle(a, gr, T, lcomp, q, 0u, my_start, L, exit_state);

  // ---- blocks before each lane's start, and the DC predictors there (an idle lane counts nothing)
  const uint32_t unit0 = (uint32_t)wg_excl_scan(L.blocks, wtot);
  int pred[3];
  for (int c = 0; c < 3; c++)
    pred[c] = wg_excl_scan(L.dc[c], wtot);

  // ---- zero the interval's blocks.  The stores are numbered in 32 bits, whose division costs a fraction of the 64-bit one: units * 8 +
  // kThreads stays below 2^32 for an interval of fewer than 2^29 - 32 blocks (64 GiB of coefficients), and this kernel has never
  // zeroed a longer one
  zero_units<uint32_t>(a.g, mcu0, 0, units, tid, kThreads);
  __threadfence_block();
  wg_sync();

  // ---- the decode proper
  uint32_t stop = 0;
  if (q.active)
    stop = write_pass(a, gr, T, lcomp, q, my_start, unit0, units, mcu0, pred, &first_err, &fin_word);
  wg_sync();
  if (first_err != kNone)
  {
    // The lanes after the one that met the interval's first error started from states of the speculating passes, which carry on past
    // such an error: what they wrote lies in blocks after the failing one and means nothing.  Those blocks go back to zero; the
    // failing block keeps the levels decoded before the error (stop < units in the lane that reported it).
    if ((uint32_t)tid == first_err >> 8)
      fail_unit = stop;
    __threadfence();
    wg_sync();
    zero_units<uint32_t>(a.g, mcu0, fail_unit + 1, units - (fail_unit + 1), tid, kThreads);
  }
  if (tid == 0)
  {
    uint32_t st = first_err != kNone ? (first_err & 0xFF) : (fin_word != kNone ? fin_word : (uint32_t)MDCT_JPEGDEC_OUT_OF_DATA);
    if (st == MDCT_JPEGDEC_OK && !last)
    {
      // the marker after the interval must be RST(k mod 8)
      const bool ok = next >= 2 && next <= len && next - 2 >= s && a.scan[next - 2] == 0xFF && a.scan[next - 1] == 0xD0 + (k & 7);
      if (!ok)
        st = MDCT_JPEGDEC_UNEXPECTED_MARKER;
    }
    a.status[k] = st;
  }
}

// ------------------------------------------------------------------------------------------------------------------ the index
// One scan's restart markers -> the offsets of its intervals (mdct_jpegdec_index; the batch library runs the same three passes over
// the chunks of many scans, each with the IndexArgs of its own scan).
struct IndexArgs
{
  const uint8_t *scan;
  uint64_t len, chunk;   // chunk: bytes per workgroup, a multiple of kThreads
  uint32_t nchunks, n_intervals;
  uint32_t *counts;      // [nchunks]: markers per chunk, then their exclusive prefix
  uint64_t *off;
};

// host: the cut of mdct_jpegdec_index: chunks of at least 4096 bytes, a multiple of kThreads, and no more of them than intervals (the
// counts live in the scan's status array)
static inline void index_chunks(uint64_t scan_len, uint64_t n_intervals, IndexArgs &a)
{
  uint64_t chunk = (scan_len + n_intervals - 1) / n_intervals;
  chunk = chunk < 4096 ? 4096 : chunk;
  a.len = scan_len;
  a.chunk = (chunk + kThreads - 1) / kThreads * kThreads;
  a.nchunks = (uint32_t)((scan_len + a.chunk - 1) / a.chunk);
  a.n_intervals = (uint32_t)n_intervals;
}

__device__ __forceinline__ bool rst_at(const uint8_t *scan, uint64_t len, uint64_t p)
{
  return scan[p] == 0xFF && p + 1 < len && (scan[p + 1] & 0xF8) == 0xD0;
}

// passes 1 (count) and 3 (WRITE) for chunk `chunk` of the scan, one workgroup of kThreads lanes
template <bool WRITE>
__device__ __forceinline__ void rst_walk(const IndexArgs &a, const uint32_t chunk)
{
  __shared__ int wtot[kThreads / 64];
  __shared__ uint32_t base;
  const uint64_t per = a.chunk / kThreads;
  const uint64_t p0 = (uint64_t)chunk * a.chunk + threadIdx.x * per;
  const uint64_t p1 = p0 + per < a.len ? p0 + per : a.len;
  int n = 0;
  for (uint64_t p = p0; p < p1; p++)
    n += rst_at(a.scan, a.len, p);
  if (!WRITE)
  {
    const int lane = threadIdx.x & 63;
    const int tot = wave_incl_scan(n, lane);
    if (lane == 63)
      wtot[threadIdx.x >> 6] = tot;
    wg_sync();
    if (threadIdx.x == 0)
      a.counts[chunk] = (uint32_t)(wtot[0] + wtot[1] + wtot[2] + wtot[3]);
    return;
  }
  if (threadIdx.x == 0)
    base = a.counts[chunk];
  const int before = wg_excl_scan(n, wtot);
  uint64_t j = (uint64_t)base + before; // ordinal of this lane's first marker
  for (uint64_t p = p0; p < p1; p++)
    if (rst_at(a.scan, a.len, p))
    {
      if (j + 1 < a.n_intervals)
        a.off[j + 1] = p + 2;
      j++;
    }
}

// pass 2 for the scan, one workgroup of 1024 lanes
__device__ __forceinline__ void rst_scan(const IndexArgs &a)
{
  __shared__ int wtot[16];
  const uint32_t total = wg1024_excl_prefix(a.counts, a.counts, a.nchunks, wtot);
  if (threadIdx.x == 0)
  {
    a.off[0] = 0;
    a.off[a.n_intervals] = a.len;
  }
  for (uint64_t j = (uint64_t)total + threadIdx.x; j + 1 < a.n_intervals; j += 1024)
    a.off[j + 1] = a.len + 2; // no marker: no data
}

} // namespace jpegdec
} // namespace mdct

// the handle mdct_jpegdec_tables_create returns (both libraries accept it)
struct mdct_jpegdec_tables
{
  mdct::jpegdec::DevTables *dev;
  int device;
  bool present[4];
};

// host: a scan descriptor's head for the decoder of scans with restart markers (marked: restart_interval > 0) or without
// (restart_interval 0); wrong_kind: the caller's message for the other kind, which may print restart_interval (%zu)
static int check_scan_head(const mdct_jpegdec_scan *d, bool marked, const char *wrong_kind)
{
  if (!d)
    return fail(MDCT_INVALID_PARAMETER, "null scan descriptor");
  if (d->n_components < 1 || d->n_components > MDCT_JPEGDEC_MAX_COMPONENTS)
    return fail(MDCT_INVALID_PARAMETER, "%d components (1..3)", d->n_components);
  if (!marked && (d->mcus_x == 0 || d->mcus_y == 0))
    return fail(MDCT_INVALID_PARAMETER, "empty MCU grid");
  if (d->mcus_x == 0 || d->mcus_y == 0 || marked != (d->restart_interval != 0))
    return fail(MDCT_INVALID_PARAMETER, wrong_kind, d->restart_interval);
  return MDCT_SUCCESS;
}

// host: ... and its components (after the head): sampling, slots, planes, block count
static int check_components(const mdct_jpegdec_scan *d)
{
  int upm = 0;
  for (int c = 0; c < d->n_components; c++)
  {
    const mdct_jpegdec_component &q = d->comp[c];
    if (q.h < 1 || q.h > 2 || q.v < 1 || q.v > 2)
      return fail(MDCT_INVALID_PARAMETER, "component %d: sampling factors %dx%d (1 or 2)", c, q.h, q.v);
    if (d->n_components == 1 && (q.h != 1 || q.v != 1))
      return fail(MDCT_INVALID_PARAMETER, "a non-interleaved scan has one block per MCU (h = v = 1)");
    if (q.dc_slot < 0 || q.dc_slot > 1 || q.ac_slot < 2 || q.ac_slot > 3)
      return fail(MDCT_INVALID_PARAMETER, "component %d: table slots %d / %d (DC 0..1, AC 2..3)", c, q.dc_slot, q.ac_slot);
    if (!q.coef || ((uintptr_t)q.coef & 15) || (q.pitch * sizeof(int16_t)) % 16)
      return fail(MDCT_INVALID_PARAMETER, "component %d: null or unaligned plane / pitch (rows must be 16-byte aligned)", c);
    if (d->mcus_x * q.h > q.blocks_x || d->mcus_y * q.v > q.blocks_y || q.pitch < q.blocks_x * 8)
      return fail(MDCT_INVALID_PARAMETER, "component %d: the MCU grid %zux%zu needs %zux%zu blocks, the plane has %zux%zu (pitch %zu)", c, d->mcus_x,
                  d->mcus_y, d->mcus_x * q.h, d->mcus_y * q.v, q.blocks_x, q.blocks_y, q.pitch);
    upm += q.h * q.v;
  }
  if (upm > MDCT_JPEGDEC_MAX_BLOCKS_PER_MCU)
    return fail(MDCT_INVALID_PARAMETER, "%d blocks per MCU (at most 10)", upm);
  if (d->mcus_x > 0xFFFFFFFFull / d->mcus_y || d->mcus_x * d->mcus_y * (size_t)upm >= (1ull << 31))
    return fail(MDCT_NOT_SUPPORTED, "more than 2^31 blocks in one scan");
  return MDCT_SUCCESS;
}

// host: DecArgs' tables and block layout from a checked descriptor; refuses a component whose table slot is empty
static int fill_geometry(const mdct_jpegdec_scan *desc, const mdct_jpegdec_tables *tables, mdct::jpegdec::DecArgs &a)
{
  a.tab = tables->dev;
  uint32_t b = 0;
  for (int c = 0; c < desc->n_components; c++)
  {
    const mdct_jpegdec_component &q = desc->comp[c];
    if (!tables->present[q.dc_slot] || !tables->present[q.ac_slot])
      return fail(MDCT_INVALID_PARAMETER, "component %d uses an empty table slot (%d / %d)", c, q.dc_slot, q.ac_slot);
    a.g.plane[c] = q.coef;
    a.g.pitch[c] = q.pitch;
    a.g.ch[c] = (uint32_t)q.h;
    a.g.cv[c] = (uint32_t)q.v;
    for (int v = 0; v < q.v; v++) // T.81 A.2.3: a component's blocks in the MCU, left to right, top to bottom
      for (int h = 0; h < q.h; h++, b++)
      {
        a.g.bcomp[b] = (uint8_t)c;
        a.g.bh[b] = (uint8_t)h;
        a.g.bv[b] = (uint8_t)v;
        a.bdc[b] = (uint8_t)q.dc_slot;
        a.bac[b] = (uint8_t)q.ac_slot;
      }
  }
  a.g.upm = b;
  a.g.mcus_x = (uint32_t)desc->mcus_x;
  a.total_mcus = (uint32_t)(desc->mcus_x * desc->mcus_y);
  return MDCT_SUCCESS;
}
