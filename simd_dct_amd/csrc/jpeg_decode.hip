// jpeg_decode.hip -- restart-marked baseline JPEG scans -> quantised int16 coefficient planes (include/mdct_jpegdec.h).
//
// Built into its own library, libmdct_jpegdec.so, linked against libmdct_hip.so; its launches go through MDCT_LAUNCH, so the launch tally
// of libmdct_hip.so (mdct_kernel_counts) counts them too.
//
//   k_rst_walk<false>  index, pass 1: one workgroup per chunk of the scan counts the RSTm markers of its chunk (into the status scratch)
//   k_rst_scan         index, pass 2: one workgroup turns the chunk counts into exclusive prefixes, writes offsets 0 / n and the missing ones
//   k_rst_walk<true>   index, pass 3: every chunk writes the offset after each of its markers at the marker's ordinal
//   k_decode           one workgroup per restart interval.  The interval's stuffed bytes are cut into kThreads sub-sequences; lane i
//                      decodes from the start of its own with a guessed state and on past its end to the first symbol boundary, whose
//                      state (bit offset past the next sub-sequence's start, coefficient index, block within the MCU) it publishes.
//                      Lane i+1 decodes again from that state while it differs from the one it started from: the Huffman code
//                      re-synchronises within a few symbols, so the exit states stop changing after a few rounds (at most kThreads:
//                      lane 0's start is exact, and each round makes one more lane exact).  Block counts and per-component DC
//                      differences are then summed over the lanes (prefix sums), the interval's blocks zeroed, and every lane decodes
//                      its sub-sequence a last time, writing its levels (Weissenberger & Schmidt, ICPP 2018).
//                      While speculating, an invalid code (skip one bit) or a run past index 63 ends the block instead of stopping
//                      the lane: a lane that stopped would publish no usable state, and the lanes after it would become exact one
//                      round at a time.  From its exact start the last pass meets the same symbols; there such an error is the
//                      interval's status.
// Byte unstuffing happens in the bit reader; positions a lane hands to the next are counted in bits after unstuffing from the next
// sub-sequence's first data byte, so both lanes count the same way.  Every loop has a bound; no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "launch_tally.h"
#include "mdct.h"
#include "mdct_jpegdec.h"
#include "wg_sync.h"

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

int hip_fail(hipError_t e, const char *what) { return fail(MDCT_NOT_SUPPORTED, "%s: %s", what, hipGetErrorString(e)); }
} // namespace

namespace mdct
{
namespace jpegdec
{

constexpr int kThreads = 256;   // lanes per restart interval
constexpr int kFastBits = 9;    // codes up to 9 bits resolve in one LDS lookup
constexpr uint32_t kErr = 0x80000000u;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// T.81 C.2 / F.2.2.3, built on the host: fast[peek9] = (length << 8) | value for codes of <= 9 bits (0: longer code or none);
// a 16-bit left-justified code c has length l if c < limit[l] (first such l), and its value is vals[(c >> (16 - l)) + delta[l]].
struct DevTables
{
  uint16_t fast[4][1 << kFastBits];
  int32_t limit[4][18];
  int32_t delta[4][18];
  uint8_t vals[4][256];
};
static_assert(sizeof(DevTables) % 4 == 0, "LDS copy in words");

struct DecArgs
{
  const uint8_t *scan;
  uint64_t scan_len;
  const uint64_t *off;
  uint32_t *status;
  const DevTables *tab;
  int16_t *plane[3];
  uint64_t pitch[3];
  uint32_t upm;                 // blocks per MCU
  uint8_t bcomp[MDCT_JPEGDEC_MAX_BLOCKS_PER_MCU], bh[MDCT_JPEGDEC_MAX_BLOCKS_PER_MCU], bv[MDCT_JPEGDEC_MAX_BLOCKS_PER_MCU];
  uint8_t bdc[MDCT_JPEGDEC_MAX_BLOCKS_PER_MCU], bac[MDCT_JPEGDEC_MAX_BLOCKS_PER_MCU];
  uint32_t ch[3], cv[3];        // h, v per component
  uint32_t mcus_x, total_mcus, restart;
  uint32_t n_intervals;
};

__constant__ uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
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
  int blocks;        // blocks completed
  int dc[3];         // sum of the DC differences per component
  uint32_t err;      // MDCT_JPEGDEC_* of a decode error (final pass)
  bool finished;     // completed the interval's last block (final pass)
  uint32_t fin;      // status after the last block: OK / LEFTOVER / UNEXPECTED_MARKER
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

// Decode from state `start` until the first symbol boundary at or after the next sub-sequence's start (a lane with a successor), the
// interval's last block (WRITE with a unit budget), or an error.  WRITE: unit0 blocks precede the start; pred = DC predictors there.
template <bool WRITE>
__device__ void run(Reader &r, const DecArgs &a, const DevTables &T, const uint32_t *lcomp, uint32_t start, Lane &out, uint32_t unit0,
                    uint32_t units, uint32_t mcu0, int pred[3], uint64_t cap)
{
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
  uint32_t mcu = 0, mx = 0, my = 0;
  int16_t *bp = nullptr;
  uint32_t comp = lcomp[b];
  if (WRITE)
  {
    mcu = mcu0 + unit / a.upm;
    my = mcu / a.mcus_x;
    mx = mcu - my * a.mcus_x;
    bp = a.plane[comp] + (size_t)(my * a.cv[comp] + a.bv[b]) * 8 * a.pitch[comp] + (size_t)(mx * a.ch[comp] + a.bh[b]) * 8;
  }
  for (uint64_t it = 0; it < cap; it++)
  {
    refill(r);
    if (r.uE != kNone && r.u >= r.uE)
    {
      out.state = ((r.u - r.uE) << 12) | (k << 4) | b;
      return;
    }
    bool block_end = false;
    const int sym = huff(r, T, k == 0 ? a.bdc[b] : a.bac[b]);
    if (sym < 0)
    {
      out.err = no_code(r);
      if (WRITE || out.err != MDCT_JPEGDEC_BAD_CODE)
        return;
      consume(r, 1); // speculating: resynchronise instead of stopping (see the kernel's comment)
      out.err = 0;
      block_end = true;
    }
    else if (k == 0)
    {
      const int s = sym;
      const int diff = extend(get_bits(r, s & 15), s & 15);
      if (overrun(r))
      {
        out.err = data_error(r);
        return;
      }
      out.dc[comp] += diff;
      if (WRITE)
      {
        pred[comp] += diff;
        bp[0] = (int16_t)pred[comp];
      }
      k = 1;
    }
    else
    {
      const int rs = sym;
      if (overrun(r))
      {
        out.err = data_error(r);
        return;
      }
      const uint32_t run_ = (uint32_t)rs >> 4, s = (uint32_t)rs & 15;
      if (s == 0)
      {
        if (run_ == 15)
        {
          k += 16;
          if (k > 64)
          {
            if (WRITE)
            {
              out.err = MDCT_JPEGDEC_COEF_OVERFLOW;
              return;
            }
            k = 64; // speculating: end the block
          }
          block_end = k == 64;
        }
        else
          block_end = true; // EOB
      }
      else
      {
        k += run_;
        if (k > 63)
        {
          if (WRITE)
          {
            out.err = MDCT_JPEGDEC_COEF_OVERFLOW;
            return;
          }
          k = 63; // speculating: keep the bit position, end the block after this level
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
          bp[(size_t)(z >> 3) * a.pitch[comp] + (z & 7)] = (int16_t)v;
        }
        k++;
        block_end = k == 64;
      }
    }
    if (block_end)
    {
      k = 0;
      out.blocks++;
      if (++b == a.upm)
        b = 0;
      comp = lcomp[b];
      if (WRITE)
      {
        if (++unit == units)
        {
          // the interval's last block: what follows must be its padding (1-bits to the byte boundary) and nothing else
          out.finished = true;
          refill(r);
          uint32_t fin = MDCT_JPEGDEC_LEFTOVER;
          if (r.dry)
          {
            const uint32_t rem = r.uend - r.u;
            if (rem < 8 && (rem == 0 || (uint32_t)(r.buf >> (64 - rem)) == (1u << rem) - 1u))
              fin = r.marker ? MDCT_JPEGDEC_UNEXPECTED_MARKER : MDCT_JPEGDEC_OK;
          }
          out.fin = fin;
          return;
        }
        if (b == 0 && ++mx == a.mcus_x)
        {
          mx = 0;
          my++;
        }
        bp = a.plane[comp] + (size_t)(my * a.cv[comp] + a.bv[b]) * 8 * a.pitch[comp] + (size_t)(mx * a.ch[comp] + a.bh[b]) * 8;
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

// exclusive prefix of x over the workgroup (kThreads lanes)
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

__global__ void __launch_bounds__(kThreads) k_decode(DecArgs a)
{
  __shared__ DevTables T;
  __shared__ uint32_t exit_state[kThreads];
  __shared__ uint32_t lcomp[16];
  __shared__ int wtot[kThreads / 64];
  __shared__ uint32_t first_err, fin_word;
  const int tid = threadIdx.x;
  const uint32_t k = blockIdx.x;
  {
    const uint32_t *src = (const uint32_t *)a.tab;
    uint32_t *dst = (uint32_t *)&T;
    for (int i = tid; i < (int)(sizeof(DevTables) / 4); i += kThreads)
      dst[i] = src[i];
    if (tid < 16)
      lcomp[tid] = tid < (int)a.upm ? a.bcomp[tid] : 0;
    if (tid == 0)
    {
      first_err = kNone;
      fin_word = kNone;
    }
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
  const uint64_t nbytes = e - s;
  uint64_t sb = (nbytes + kThreads - 1) / kThreads;
  sb = sb < 8 ? 8 : sb;
  const uint32_t nact = nbytes ? (uint32_t)((nbytes + sb - 1) / sb) : 1u;
  const uint32_t mcu0 = k * a.restart;
  const uint32_t nmcu = (a.total_mcus - mcu0) < a.restart ? a.total_mcus - mcu0 : a.restart;
  const uint32_t units = nmcu * a.upm;
  const bool active = (uint32_t)tid < nact;
  const uint64_t s0 = s + (uint64_t)tid * sb;
  const uint64_t E = (uint32_t)tid + 1 < nact ? s0 + sb : ~uint64_t(0);
  const uint64_t cap = 8 * (e - (s0 < e ? s0 : e)) + 64;
  wg_sync();

  // ---- synchronisation: lane 0 starts exact, the others from a guess, until no start changes
  Lane L;
  Reader r;
  uint32_t my_start = 0;
  int dummy[3] = {0, 0, 0};
  if (active)
  {
    reader_init(r, a, s0, e, E, tid == 0);
    run<false>(r, a, T, lcomp, my_start, L, 0, 0, 0, dummy, cap);
  }
  else
  {
    L.state = kErr;
    L.blocks = 0;
    L.dc[0] = L.dc[1] = L.dc[2] = 0;
  }
  exit_state[tid] = L.state;
  for (uint32_t round = 0; round <= nact; round++)
  {
    wg_sync();
    const uint32_t want = tid == 0 ? 0u : exit_state[tid - 1];
    const bool changed = active && want != my_start;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (!__syncthreads_or(changed))
      break;
    if (changed)
    {
      my_start = want;
      reader_init(r, a, s0, e, E, tid == 0);
      run<false>(r, a, T, lcomp, my_start, L, 0, 0, 0, dummy, cap);
      exit_state[tid] = L.state;
    }
  }

  // ---- blocks before each lane's start, and the DC predictors there
  const int unit0 = wg_excl_scan(active ? L.blocks : 0, wtot);
  int pred[3];
  for (int c = 0; c < 3; c++)
    pred[c] = wg_excl_scan(active ? L.dc[c] : 0, wtot);

  // ---- zero the interval's blocks (consecutive lanes: consecutive blocks of one MCU row, same pixel row)
  for (uint32_t wi = tid; wi < units * 8; wi += kThreads)
  {
    const uint32_t unit = wi % units, row = wi / units;
    const uint32_t mcu = mcu0 + unit / a.upm, b = unit % a.upm, c = a.bcomp[b];
    const uint32_t my = mcu / a.mcus_x, mx = mcu - my * a.mcus_x;
    int16_t *p = a.plane[c] + ((size_t)(my * a.cv[c] + a.bv[b]) * 8 + row) * a.pitch[c] + (size_t)(mx * a.ch[c] + a.bh[b]) * 8;
    *(uint4 *)p = make_uint4(0, 0, 0, 0);
  }
  __threadfence_block();
  wg_sync();

  // ---- the decode proper
  if (active)
  {
    reader_init(r, a, s0, e, E, tid == 0);
    Lane F;
    run<true>(r, a, T, lcomp, my_start, F, (uint32_t)unit0, units, mcu0, pred, cap);
    if (F.err && (uint32_t)unit0 < units)
      atomicMin(&first_err, ((uint32_t)tid << 8) | F.err);
    if (F.finished)
      fin_word = F.fin;
  }
  wg_sync();
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
struct IndexArgs
{
  const uint8_t *scan;
  uint64_t len, chunk;   // chunk: bytes per workgroup, a multiple of kThreads
  uint32_t nchunks, n_intervals;
  uint32_t *counts;      // [nchunks]: markers per chunk, then their exclusive prefix
  uint64_t *off;
};

__device__ __forceinline__ bool rst_at(const uint8_t *scan, uint64_t len, uint64_t p)
{
  return scan[p] == 0xFF && p + 1 < len && (scan[p + 1] & 0xF8) == 0xD0;
}

template <bool WRITE>
__global__ void __launch_bounds__(kThreads) k_rst_walk(IndexArgs a)
{
  __shared__ int wtot[kThreads / 64];
  __shared__ uint32_t base;
  const uint64_t per = a.chunk / kThreads;
  const uint64_t p0 = (uint64_t)blockIdx.x * a.chunk + threadIdx.x * per;
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
      a.counts[blockIdx.x] = (uint32_t)(wtot[0] + wtot[1] + wtot[2] + wtot[3]);
    return;
  }
  if (threadIdx.x == 0)
    base = a.counts[blockIdx.x];
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

__global__ void __launch_bounds__(1024) k_rst_scan(IndexArgs a)
{
  __shared__ int wtot[16];
  const uint32_t per = (a.nchunks + 1023) / 1024;
  const uint32_t c0 = threadIdx.x * per, c1 = c0 + per < a.nchunks ? c0 + per : a.nchunks;
  uint32_t n = 0;
  for (uint32_t c = c0; c < c1; c++)
    n += a.counts[c];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int inc = wave_incl_scan((int)n, lane);
  if (lane == 63)
    wtot[w] = inc;
  wg_sync();
  int wb = 0, total = 0;
  for (int j = 0; j < 16; j++)
  {
    wb += j < w ? wtot[j] : 0;
    total += wtot[j];
  }
  uint32_t run_ = (uint32_t)(wb + inc) - n;
  for (uint32_t c = c0; c < c1; c++)
  {
    const uint32_t m = a.counts[c];
    a.counts[c] = run_;
    run_ += m;
  }
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

using namespace mdct::jpegdec;

struct mdct_jpegdec_tables
{
  DevTables *dev;
  int device;
  bool present[4];
};

static int build_tables(const uint8_t *const bits16[4], const uint8_t *const vals[4], const int nvals[4], DevTables *out, bool present[4])
{
  if (!bits16 || !vals || !nvals)
    return fail(MDCT_INVALID_PARAMETER, "null table arrays");
  if (out)
    memset(out, 0, sizeof(*out));
  for (int t = 0; t < 4; t++)
  {
    present[t] = bits16[t] != nullptr;
    if (!present[t])
      continue;
    if (!vals[t] && nvals[t] > 0)
      return fail(MDCT_INVALID_PARAMETER, "slot %d: null values", t);
    if (nvals[t] < 0 || nvals[t] > 256)
      return fail(MDCT_INVALID_PARAMETER, "slot %d: %d values (at most 256)", t, nvals[t]);
    int total = 0;
    for (int l = 0; l < 16; l++)
      total += bits16[t][l];
    if (total != nvals[t])
      return fail(MDCT_INVALID_PARAMETER, "slot %d: the 16 counts add up to %d codes, %d values given", t, total, nvals[t]);
    for (int i = 0; i < total; i++)
    {
      const int v = vals[t][i];
      if (t < 2 ? v > 11 : (v & 15) > 10)
        return fail(MDCT_INVALID_PARAMETER, "slot %d: value 0x%02x is not a baseline %s symbol", t, v, t < 2 ? "DC" : "AC");
    }
    // canonical codes (C.2); no code may be all 1-bits, as libjpeg requires
    int code = 0, p = 0;
    for (int l = 1; l <= 16; l++)
    {
      const int n = bits16[t][l - 1];
      if (out)
      {
        out->limit[t][l] = n ? (code + n) << (16 - l) : 0;
        out->delta[t][l] = p - code;
        if (l <= kFastBits)
          for (int i = 0; i < n; i++)
            for (int f = (code + i) << (kFastBits - l); f < (code + i + 1) << (kFastBits - l); f++)
              out->fast[t][f] = (uint16_t)((l << 8) | vals[t][p + i]);
      }
      code += n;
      p += n;
      if (code >= (1 << l))
        return fail(MDCT_INVALID_PARAMETER, "slot %d: codes over-subscribed at length %d", t, l);
      code <<= 1;
    }
    if (out)
    {
      out->limit[t][17] = 0x7FFFFFFF;
      memcpy(out->vals[t], vals[t], (size_t)total);
    }
  }
  return MDCT_SUCCESS;
}

extern "C" {

const char *mdct_jpegdec_last_error(void) { return g_err; }

int mdct_jpegdec_tables_check(const uint8_t *const bits16[4], const uint8_t *const vals[4], const int nvals[4])
{
  bool present[4];
  return build_tables(bits16, vals, nvals, nullptr, present);
}

int mdct_jpegdec_tables_create(mdct_jpegdec_tables **tables, const uint8_t *const bits16[4], const uint8_t *const vals[4], const int nvals[4])
{
  if (!tables)
    return fail(MDCT_INVALID_PARAMETER, "null tables");
  *tables = nullptr;
  DevTables host;
  bool present[4];
  int rc = build_tables(bits16, vals, nvals, &host, present);
  if (rc)
    return rc;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess)
    return hip_fail(e, "hipGetDevice");
  DevTables *d = nullptr;
  if ((e = hipMalloc(&d, sizeof(DevTables))) != hipSuccess)
    return hip_fail(e, "hipMalloc");
  if ((e = hipMemcpy(d, &host, sizeof(DevTables), hipMemcpyHostToDevice)) != hipSuccess)
  {
    (void)hipFree(d);
    return hip_fail(e, "hipMemcpy");
  }
  mdct_jpegdec_tables *t = new mdct_jpegdec_tables;
  t->dev = d;
  t->device = dev;
  memcpy(t->present, present, sizeof(present));
  *tables = t;
  return MDCT_SUCCESS;
}

int mdct_jpegdec_tables_destroy(mdct_jpegdec_tables *tables)
{
  if (!tables)
    return MDCT_SUCCESS;
  const hipError_t e = hipFree(tables->dev);
  delete tables;
  return e == hipSuccess ? MDCT_SUCCESS : hip_fail(e, "hipFree");
}

static int check_desc(const mdct_jpegdec_scan *d, size_t *n_intervals)
{
  if (!d)
    return fail(MDCT_INVALID_PARAMETER, "null scan descriptor");
  if (d->n_components < 1 || d->n_components > MDCT_JPEGDEC_MAX_COMPONENTS)
    return fail(MDCT_INVALID_PARAMETER, "%d components (1..3)", d->n_components);
  if (d->mcus_x == 0 || d->mcus_y == 0 || d->restart_interval == 0)
    return fail(MDCT_INVALID_PARAMETER, "empty MCU grid or restart interval 0 (scans without restart markers are not supported)");
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
  *n_intervals = (d->mcus_x * d->mcus_y + d->restart_interval - 1) / d->restart_interval;
  return MDCT_SUCCESS;
}

size_t mdct_jpegdec_intervals(const mdct_jpegdec_scan *desc)
{
  size_t n = 0;
  return check_desc(desc, &n) ? 0 : n;
}

int mdct_jpegdec_index(const uint8_t *scan, size_t scan_len, size_t n_intervals, uint64_t *interval_offsets, uint32_t *interval_status, void *stream)
{
  if (!interval_offsets || !interval_status || (!scan && scan_len))
    return fail(MDCT_INVALID_PARAMETER, "null scan / offsets / status");
  if (n_intervals == 0 || n_intervals >= (1ull << 31))
    return fail(MDCT_INVALID_PARAMETER, "%zu intervals", n_intervals);
  IndexArgs a;
  a.scan = scan;
  a.len = scan_len;
  uint64_t chunk = (scan_len + n_intervals - 1) / n_intervals;
  chunk = chunk < 4096 ? 4096 : chunk;
  a.chunk = (chunk + kThreads - 1) / kThreads * kThreads;
  a.nchunks = (uint32_t)((scan_len + a.chunk - 1) / a.chunk); // <= n_intervals: the counts fit in the status array
  a.n_intervals = (uint32_t)n_intervals;
  a.counts = interval_status;
  a.off = interval_offsets;
  hipStream_t s = (hipStream_t)stream;
  if (a.nchunks)
    MDCT_LAUNCH(k_rst_walk<false>, dim3(a.nchunks), dim3(kThreads), 0, s, a);
  MDCT_LAUNCH(k_rst_scan, dim3(1), dim3(1024), 0, s, a);
  if (a.nchunks)
    MDCT_LAUNCH(k_rst_walk<true>, dim3(a.nchunks), dim3(kThreads), 0, s, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : hip_fail(e, "index launch");
}

int mdct_jpegdec_decode(const mdct_jpegdec_scan *desc, const mdct_jpegdec_tables *tables, const uint8_t *scan, size_t scan_len,
                        const uint64_t *interval_offsets, uint32_t *interval_status, void *stream)
{
  size_t n = 0;
  int rc = check_desc(desc, &n);
  if (rc)
    return rc;
  if (!tables || !interval_offsets || !interval_status || (!scan && scan_len))
    return fail(MDCT_INVALID_PARAMETER, "null tables / scan / offsets / status");
  DecArgs a;
  memset(&a, 0, sizeof(a));
  a.scan = scan;
  a.scan_len = scan_len;
  a.off = interval_offsets;
  a.status = interval_status;
  a.tab = tables->dev;
  uint32_t b = 0;
  for (int c = 0; c < desc->n_components; c++)
  {
    const mdct_jpegdec_component &q = desc->comp[c];
    if (!tables->present[q.dc_slot] || !tables->present[q.ac_slot])
      return fail(MDCT_INVALID_PARAMETER, "component %d uses an empty table slot (%d / %d)", c, q.dc_slot, q.ac_slot);
    a.plane[c] = q.coef;
    a.pitch[c] = q.pitch;
    a.ch[c] = (uint32_t)q.h;
    a.cv[c] = (uint32_t)q.v;
    for (int v = 0; v < q.v; v++) // T.81 A.2.3: a component's blocks in the MCU, left to right, top to bottom
      for (int h = 0; h < q.h; h++, b++)
      {
        a.bcomp[b] = (uint8_t)c;
        a.bh[b] = (uint8_t)h;
        a.bv[b] = (uint8_t)v;
        a.bdc[b] = (uint8_t)q.dc_slot;
        a.bac[b] = (uint8_t)q.ac_slot;
      }
  }
  a.upm = b;
  a.mcus_x = (uint32_t)desc->mcus_x;
  a.total_mcus = (uint32_t)(desc->mcus_x * desc->mcus_y);
  a.restart = (uint32_t)(desc->restart_interval < a.total_mcus ? desc->restart_interval : a.total_mcus);
  a.n_intervals = (uint32_t)n;
  MDCT_LAUNCH(k_decode, dim3((uint32_t)n), dim3(kThreads), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : hip_fail(e, "decode launch");
}

} // extern "C"
