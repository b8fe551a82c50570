// jpeg_decode_progressive.hip -- the scans of a progressive JPEG (T.81 Annex G: spectral selection and successive approximation), one
// restart interval per workgroup -> quantised int16 coefficient planes (include/mdct_jpegdec_prog.h).
//
// Built into its own library, libmdct_jpegdec_prog.so, linked against libmdct_jpegdec.so (whose table handle, descriptor and interval
// index it takes) and libmdct_hip.so (whose launch tally counts its launches).
//
//   k_decode_prog_dc   a DC-first scan (ss = se = 0), one workgroup per restart interval
//   k_decode_prog_ac   an AC-band scan (1 <= ss <= se <= 63, one component), one workgroup per restart interval
//
// Both are k_decode's model (jpeg_decode.hip) over another symbol grammar, Band<AC>, and made of jpegdec_common.h's pieces: the bit
// reader, the Huffman lookup, run, speculate, settle and write_pass, the interval's bookkeeping (interval_of, put_status,
// after_last_block), the table load and the prefix sum.  This file's own are the clamped prefix of the block counts (first_unit),
// decode_interval<AC> and the refinement scans.
//
// The state between two symbols is k_decode's: k is 0 in a DC scan and ss..se in an AC band, whose block in MCU is 0.  An end-of-band
// run is accounted whole where its EOBn is decoded, so the prefix sum of the block counts is exact (a garbage EOBn is simply counted).
// There is no zeroing pass: the caller's planes are zero in the band, and only an interval that fails sets the band's positions of the
// blocks behind the failing one back to zero (the lanes behind the error wrote levels of the re-synchronised decode there).
//
// Successive approximation (ProgArgs::ah, al, uniform per launch) adds three scan kinds to the two kernels as runtime branches:
//   a first scan with al > 0 is the path above, its levels stored shifted left by al;
//   a DC refinement scan (k_decode_prog_dc, ah > 0) is one raw bit per block and no Huffman code: refine_dc gives every lane the bits
//   of its own sub-sequence by a workgroup prefix sum of the unstuffed data bytes before it, with no speculation and no settle();
//   an AC refinement scan (k_decode_prog_ac, ah > 0) is decoded sequentially, one interval per ONE-WAVE workgroup (refine_ac): how
//   many bits a symbol consumes depends on which coefficients of the block earlier scans left non-zero, so a lane that does not know
//   its block cannot decode and the sub-sequence scheme does not apply.  The wave loads the block (lane i the band's zig-zag
//   position i), three ballots hand lane 0 the block's history as 64-bit masks, lane 0 decodes the block's symbols and correction
//   bits on those masks alone, and the wave applies and stores what changed.
// A refinement interval that fails is left as it is (zeroing would destroy what earlier scans decoded).
// Every loop has a bound; no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "jpegdec_common.h"
#include "launch_tally.h"
#include "mdct_jpegdec_prog.h"

namespace mdct
{
namespace jpegdec
{
namespace prog
{

struct ProgArgs
{
  DecArgs d;
  uint32_t ss, se; // the band, zig-zag
  uint32_t ah, al; // successive approximation (G.1.2): ah = 0 a first scan, ah = al + 1 a refinement; levels count in units of 1 << al
};

// blocks before each lane's start.  A lane's count is clamped to units + 1 and the sum too, so that counts of garbage (lanes behind an
// error, whose end-of-band runs mean nothing) can neither wrap nor bring a later lane back inside the interval; the counts are summed
// in two 16-bit halves, each of which stays far inside wg_excl_scan's int.
__device__ __forceinline__ uint32_t first_unit(uint32_t blocks, uint32_t units, int *wtot)
{
  const uint32_t c = blocks < units + 1 ? blocks : units + 1; // units < 2^31
  const uint64_t lo = (uint32_t)wg_excl_scan((int)(c & 0xFFFFu), wtot), hi = (uint32_t)wg_excl_scan((int)(c >> 16), wtot);
  const uint64_t sum = (hi << 16) + lo;
  return sum < (uint64_t)units + 1 ? (uint32_t)sum : units + 1;
}

// ------------------------------------------------------------------------------------------------------ DC refinement (G.1.2.1)
// One raw bit per block in the scan's block order; a set bit ORs 1 << al into position (0, 0).  Every bit is a symbol boundary, so
// nothing is speculated: lane i counts the unstuffed data bytes of its sub-sequence, a prefix sum gives it the number of its first
// data byte (bit 8 * that is its first block), and it reads its bytes again and writes.  A 0xFF 0x00 pair may straddle the cut: the
// 0xFF's lane counts the pair, the next lane skips the zero.  A marker ends the data: the lanes behind its lane write nothing.
// mark / bad / total: three words of LDS.
__device__ __forceinline__ void refine_dc(const ProgArgs &a, uint32_t *lcomp, int *wtot, uint32_t *mark, uint32_t *bad, uint32_t *total)
{
  const int tid = threadIdx.x;
  const uint32_t k = blockIdx.x;
  const BlockPlace &g = a.d.g;
  if (tid < 16)
    lcomp[tid] = tid < (int)g.upm ? g.bcomp[tid] : 0;
  if (tid == 0)
  {
    *mark = kNone;
    *bad = 0;
    *total = 0;
  }
  const Interval iv = interval_of(a.d, k);
  const uint64_t s = iv.s, e = iv.e, sb = iv.sb;
  const uint32_t units = iv.units;
  const uint32_t need = units / 8 + 1; // data bytes that matter: one more than the blocks' means bits left over
  uint64_t p0 = s + (uint64_t)tid * sb;
  p0 = p0 < e ? p0 : e;
  const uint64_t p1 = e - p0 > sb ? p0 + sb : e;
  if (tid > 0 && p0 < p1 && a.d.scan[p0] == 0 && a.d.scan[p0 - 1] == 0xFF)
    p0++; // the stuffed zero of the previous lane's last byte
  wg_sync();

  // ---- the data bytes of each sub-sequence, up to a marker
  uint32_t cnt = 0;
  bool marker = false;
  for (uint64_t p = p0; p < p1 && cnt <= need; p++)
  {
    if (a.d.scan[p] == 0xFF)
    {
      if (p + 1 < e && a.d.scan[p + 1] == 0)
        p++;
      else
      {
        marker = true;
        break;
      }
    }
    cnt++;
  }
  if (marker)
    atomicMin(mark, (uint32_t)tid);
  wg_sync();
  const uint32_t mlane = *mark;
  const bool dead = (uint32_t)tid > mlane;
  if (dead)
    cnt = 0;
  const uint32_t byte0 = first_unit(cnt, need + 1, wtot); // (clamped to need + 2: beyond that nothing is told apart)
  if (tid == kThreads - 1)
    *total = byte0 + cnt < need + 2 ? byte0 + cnt : need + 2;

  // ---- the bits
  if (!dead)
  {
    uint64_t j = byte0; // number of the data byte
    for (uint64_t p = p0; p < p1 && 8 * j < units; p++, j++)
    {
      const uint32_t byte = a.d.scan[p];
      if (byte == 0xFF)
      {
        if (p + 1 < e && a.d.scan[p + 1] == 0)
          p++;
        else
          break;
      }
      const uint32_t u0 = (uint32_t)(8 * j), n = units - u0 < 8 ? units - u0 : 8;
      const uint32_t mcu = iv.mcu0 + u0 / g.upm;
      uint32_t b = u0 % g.upm, my = mcu / g.mcus_x, mx = mcu - my * g.mcus_x;
      for (uint32_t t = 0; t < n; t++)
      {
        if ((byte >> (7 - t)) & 1)
        {
          int16_t *bp = block_at(g, mx, my, b, lcomp[b], 0);
          bp[0] = (int16_t)(bp[0] | (1 << a.al));
        }
        if (++b == g.upm)
        {
          b = 0;
          if (++mx == g.mcus_x)
          {
            mx = 0;
            my++;
          }
        }
      }
      if (n < 8 && (byte & (0xFFu >> n)) != (0xFFu >> n)) // the padding after the last block's bit: 1-bits
        *bad = 1;
    }
  }
  wg_sync();
  if (tid == 0)
  {
    const uint64_t bits = 8ull * *total;
    const uint32_t broken = mlane != kNone ? MDCT_JPEGDEC_UNEXPECTED_MARKER : MDCT_JPEGDEC_OUT_OF_DATA;
    const uint32_t st = bits < units ? broken : (bits - units >= 8 || *bad) ? MDCT_JPEGDEC_LEFTOVER : mlane != kNone ? broken : MDCT_JPEGDEC_OK;
    put_status(a.d, iv, k, st);
  }
}

// ------------------------------------------------------------------------------------------------------ AC refinement (G.1.2.3)
// Lane 0: the symbols and correction bits of one block (Figure G.7) on the block's history: bit i of nz says that zig-zag position i
// is non-zero.  eobrun: blocks of a running end-of-band run, this one included; left: blocks the interval has from this one on.
// -> add: positions whose correction bit is set; nw / nwneg: positions of new coefficients and which of them are negative.
// Returns 0 or the MDCT_JPEGDEC_* that stops the interval.  Every trip of every loop moves k on, and k ends at se.
__device__ __forceinline__ uint32_t refine_block(Reader &r, const DevTables &T, int t, uint32_t ss, uint32_t se, uint64_t nz, uint32_t &eobrun,
                                                 uint32_t left, uint64_t &add, uint64_t &nw, uint64_t &nwneg)
{
  uint32_t k = ss;
  if (eobrun == 0)
  {
    while (k <= se)
    {
      refill(r);
      const int sym = huff(r, T, t);
      if (sym < 0)
        return no_code(r);
      if (overrun(r))
        return data_error(r);
      uint32_t run_ = (uint32_t)sym >> 4;
      const uint32_t sz = (uint32_t)sym & 15;
      uint32_t negative = 0;
      if (sz > 1)
        return MDCT_JPEGDEC_BAD_CODE; // a refinement scan codes one bit of a new coefficient
      if (sz == 1)
        negative = get_bits(r, 1) ^ 1u;
      else if (run_ != 15) // EOBn
      {
        const uint32_t n = (1u << run_) + get_bits(r, run_);
        if (overrun(r))
          return data_error(r);
        if (n > left)
          return MDCT_JPEGDEC_EOBRUN_OVERFLOW;
        eobrun = n;
        break;
      }
      if (overrun(r))
        return data_error(r);
      // over run_ positions without history; every position with history on the way takes a correction bit
      bool placed = false;
      for (; k <= se; k++)
      {
        if ((nz >> k) & 1)
        {
          refill(r);
          if (get_bits(r, 1))
            add |= 1ull << k;
        }
        else if (run_ == 0)
        {
          placed = true;
          break;
        }
        else
          run_--;
      }
      if (overrun(r))
        return data_error(r);
      if (!placed)
        return MDCT_JPEGDEC_COEF_OVERFLOW; // the run (a ZRL's sixteenth position too) ends past se
      if (sz)
      {
        nw |= 1ull << k;
        nwneg |= (uint64_t)negative << k;
      }
      k++;
    }
  }
  if (eobrun > 0)
  {
    // the rest of the band: correction bits of the positions with history
    uint64_t m = k <= se ? nz & ((~0ull >> (63 - se)) & (~0ull << k)) : 0;
    while (m)
    {
      const uint32_t i = (uint32_t)__builtin_ctzll(m);
      m &= m - 1;
      refill(r);
      if (get_bits(r, 1))
        add |= 1ull << i;
    }
    if (overrun(r))
      return data_error(r);
    eobrun--;
  }
  return 0;
}

__device__ __forceinline__ uint64_t from_lane0(uint64_t x)
{
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)x, 0, 64), hi = (uint32_t)__shfl((int)(uint32_t)(x >> 32), 0, 64);
  return ((uint64_t)hi << 32) | lo;
}

// One interval of an AC refinement scan by a workgroup of ONE wave (the launch gives it 64 lanes).  Lane i holds zig-zag position i of
// the current block; the next block's load is in flight while lane 0 decodes.
__device__ __forceinline__ void refine_ac(const ProgArgs &a, DevTables &T, uint32_t *lcomp)
{
  const uint32_t tid = threadIdx.x, k = blockIdx.x;
  const BlockPlace &g = a.d.g;
  load_tables(a.d, T, lcomp, (int)tid, 64);
  const Interval iv = interval_of(a.d, k);
  wg_sync();
  const uint32_t comp = g.bcomp[0], units = iv.units;
  const int p1 = 1 << a.al;
  const bool inband = tid >= a.ss && tid <= a.se && tid < 64;
  const uint32_t z = kZigzag[tid & 63];
  const size_t zoff = (size_t)(z >> 3) * g.pitch[comp] + (z & 7);
  Reader r;
  reader_init(r, a.d, iv.s, iv.e, ~uint64_t(0), true);
  uint32_t eobrun = 0, st = 0;
  uint32_t my = iv.mcu0 / g.mcus_x, mx = iv.mcu0 - my * g.mcus_x;
  int16_t *bp = block_at(g, mx, my, 0, comp, 0);
  int coef = inband && units ? bp[zoff] : 0;
  for (uint32_t unit = 0; unit < units; unit++)
  {
    int16_t *bq = bp;
    int coming = 0;
    if (unit + 1 < units)
    {
      if (++mx == g.mcus_x)
      {
        mx = 0;
        my++;
      }
      bq = block_at(g, mx, my, 0, comp, 0);
      coming = inband ? bq[zoff] : 0;
    }
    const uint64_t nz = __ballot(coef != 0);
    uint64_t add = 0, nw = 0, nwneg = 0;
    if (tid == 0)
      st = refine_block(r, T, a.d.bac[0], a.ss, a.se, nz, eobrun, units - unit, add, nw, nwneg);
    add = from_lane0(add);
    nw = from_lane0(nw);
    nwneg = from_lane0(nwneg);
    st = (uint32_t)__shfl((int)st, 0, 64);
    if (inband)
    {
      if (coef != 0)
      {
        if (((add >> tid) & 1) && (coef & p1) == 0) // away from zero, where this bit is still clear
          bp[zoff] = (int16_t)(coef + (coef < 0 ? -p1 : p1));
      }
      else if ((nw >> tid) & 1)
        bp[zoff] = (int16_t)(((nwneg >> tid) & 1) ? -p1 : p1);
    }
    if (st)
      break;
    bp = bq;
    coef = coming;
  }
  if (tid == 0)
    put_status(a.d, iv, k, st ? st : units ? after_last_block(r) : (uint32_t)MDCT_JPEGDEC_OUT_OF_DATA);
}

template <bool AC>
__device__ __forceinline__ void decode_interval(const ProgArgs &a, DevTables &T, uint32_t *exit_state, uint32_t *lcomp, int *wtot,
                                                uint32_t *first_err, uint32_t *fin_word, uint32_t *fail_unit)
{
  const int tid = threadIdx.x;
  const uint32_t k = blockIdx.x;
  const Band<AC> gr{a.ss, a.se, a.al};
  load_tables(a.d, T, lcomp, tid);
  if (tid == 0)
  {
    *first_err = kNone;
    *fin_word = kNone;
  }
  const Interval iv = interval_of(a.d, k);
  const SubLane q = sub_lane(iv.s, iv.e, iv.sb, tid, true);
  const uint32_t mcu0 = iv.mcu0, units = iv.units;
  wg_sync();

  // ---- synchronisation: lane 0 starts exact (the band's first position of an MCU's first block), the others from the same guess
  Lane L;
  const uint32_t want0 = a.ss << 4;
  uint32_t my_start = want0;
  speculate(a.d, gr, T, lcomp, q, my_start, L);
  settle(a.d, gr, T, lcomp, q, want0, my_start, L, exit_state);

  // ---- blocks before each lane's start, and the DC predictors there
  const uint32_t unit0 = first_unit((uint32_t)L.blocks, units, wtot);
  int pred[3] = {0, 0, 0};
  if (!AC)
    for (int c = 0; c < 3; c++)
      pred[c] = wg_excl_scan(L.dc[c], wtot);

  // ---- the decode proper
  uint32_t stop = 0;
  if (q.active)
    stop = write_pass(a.d, gr, T, lcomp, q, my_start, unit0, units, mcu0, pred, first_err, fin_word);
  wg_sync();
  if (*first_err != kNone)
  {
    // The lanes after the one that met the interval's first error started from states of the speculating passes, which carry on past
    // such an error: what they wrote lies in blocks after the failing one (every speculated error ends its block) and means nothing.
    // The band's positions of those blocks go back to zero, as scattered stores: this path is rare.
    if ((uint32_t)tid == *first_err >> 8)
      *fail_unit = stop;
    __threadfence();
    wg_sync();
    const uint32_t z0 = *fail_unit + 1, band = a.se - a.ss + 1;
    const uint64_t n = z0 < units ? (uint64_t)(units - z0) * band : 0;
    for (uint64_t i = tid; i < n; i += kThreads)
    {
      const uint32_t unit = z0 + (uint32_t)(i / band), z = kZigzag[a.ss + (uint32_t)(i % band)];
      const uint32_t mcu = mcu0 + unit / a.d.g.upm, b = unit % a.d.g.upm, my = mcu / a.d.g.mcus_x, c = lcomp[b];
      block_at(a.d.g, mcu - my * a.d.g.mcus_x, my, b, c, 0)[(size_t)(z >> 3) * a.d.g.pitch[c] + (z & 7)] = 0;
    }
  }
  if (tid == 0)
  {
    const uint32_t st = *first_err != kNone ? (*first_err & 0xFF) : (*fin_word != kNone ? *fin_word : (uint32_t)MDCT_JPEGDEC_OUT_OF_DATA);
    put_status(a.d, iv, k, st);
  }
}

#define MDCT_PROG_KERNEL(name, AC)                                                                                                        \
  __global__ void __launch_bounds__(kThreads) name(ProgArgs a)                                                                            \
  {                                                                                                                                       \
    __shared__ DevTables T;                                                                                                               \
    __shared__ uint32_t exit_state[kThreads];                                                                                             \
    __shared__ uint32_t lcomp[16];                                                                                                        \
    __shared__ int wtot[kThreads / 64];                                                                                                   \
    __shared__ uint32_t first_err, fin_word, fail_unit;                                                                                   \
    if (a.ah) /* a refinement scan (uniform) */                                                                                           \
    {                                                                                                                                     \
      if (AC)                                                                                                                             \
        refine_ac(a, T, lcomp);                                                                                                           \
      else                                                                                                                                \
        refine_dc(a, lcomp, wtot, &first_err, &fin_word, &fail_unit);                                                                     \
      return;                                                                                                                             \
    }                                                                                                                                     \
    decode_interval<AC>(a, T, exit_state, lcomp, wtot, &first_err, &fin_word, &fail_unit);                                                \
  }

MDCT_PROG_KERNEL(k_decode_prog_dc, false)
MDCT_PROG_KERNEL(k_decode_prog_ac, true)

} // namespace prog
} // namespace jpegdec
} // namespace mdct

using namespace mdct::jpegdec;

// host: the descriptor for the band (ss, se).  The slot class the band does not use is ignored: `d` is the caller's descriptor with
// those slots set to legal values, so that check_components (and fill_geometry) can be applied as they are.
static int check_prog(const mdct_jpegdec_scan *desc, int ss, int se, mdct_jpegdec_scan &d, size_t *n_intervals)
{
  int rc = check_scan_head(desc, true, "empty MCU grid or restart interval 0 (progressive scans without restart markers are not supported)");
  if (rc)
    return rc;
  const bool dc = ss == 0 && se == 0, ac = 1 <= ss && ss <= se && se <= 63;
  if (!dc && !ac)
    return fail(MDCT_INVALID_PARAMETER, "band %d..%d (0..0: the DC scan; 1 <= ss <= se <= 63: an AC band)", ss, se);
  if (ac && (desc->n_components != 1 || desc->comp[0].h != 1 || desc->comp[0].v != 1))
    return fail(MDCT_INVALID_PARAMETER, "an AC band takes one component with h = v = 1 (T.81 G.1.1.1.1)");
  d = *desc;
  for (int c = 0; c < d.n_components; c++)
    (dc ? d.comp[c].ac_slot : d.comp[c].dc_slot) = dc ? 2 : 0;
  if ((rc = check_components(&d)))
    return rc;
  *n_intervals = (d.mcus_x * d.mcus_y + d.restart_interval - 1) / d.restart_interval;
  return MDCT_SUCCESS;
}

extern "C" {

const char *mdct_jpegdec_prog_last_error(void) { return g_err; }

size_t mdct_jpegdec_prog_intervals(const mdct_jpegdec_scan *desc, int ss, int se)
{
  mdct_jpegdec_scan d;
  size_t n = 0;
  return check_prog(desc, ss, se, d, &n) ? 0 : n;
}

int mdct_jpegdec_prog_decode_approx(const mdct_jpegdec_scan *desc, int ss, int se, int ah, int al, const mdct_jpegdec_tables *tables,
                                    const uint8_t *scan, size_t scan_len, const uint64_t *interval_offsets, uint32_t *interval_status, void *stream)
{
  mdct_jpegdec_scan d;
  size_t n = 0;
  int rc = check_prog(desc, ss, se, d, &n);
  if (rc)
    return rc;
  if (al < 0 || al > 13)
    return fail(MDCT_INVALID_PARAMETER, "successive approximation: Al %d (0..13)", al);
  if (ah != 0 && ah != al + 1)
    return fail(MDCT_INVALID_PARAMETER, "successive approximation: Ah %d with Al %d (0: a first scan; Al + 1: a refinement scan)", ah, al);
  const bool ac = ss > 0, no_table = !ac && ah != 0; // a DC refinement scan is raw bits
  if ((!tables && !no_table) || !interval_offsets || !interval_status || (!scan && scan_len))
    return fail(MDCT_INVALID_PARAMETER, "null tables / scan / offsets / status");
  // only the slots of the band's class must be present: the other class counts as present for fill_geometry and is never read
  mdct_jpegdec_tables used;
  memset(&used, 0, sizeof(used));
  if (tables)
    used = *tables;
  for (int t = 0; t < 4; t++)
    if ((t >= 2) != ac || no_table)
      used.present[t] = true;
  prog::ProgArgs a;
  memset(&a, 0, sizeof(a));
  a.d.scan = scan;
  a.d.scan_len = scan_len;
  a.d.off = interval_offsets;
  a.d.status = interval_status;
  if ((rc = fill_geometry(&d, &used, a.d)))
    return rc;
  a.d.restart = (uint32_t)(d.restart_interval < a.d.total_mcus ? d.restart_interval : a.d.total_mcus);
  a.d.n_intervals = (uint32_t)n;
  a.ss = (uint32_t)ss;
  a.se = (uint32_t)se;
  a.ah = (uint32_t)ah;
  a.al = (uint32_t)al;
  if (ac) // a refinement scan: one wave per interval, whose lane 0 decodes (refine_ac)
    MDCT_LAUNCH(prog::k_decode_prog_ac, dim3((uint32_t)n), dim3(ah ? 64 : kThreads), 0, (hipStream_t)stream, a);
  else
    MDCT_LAUNCH(prog::k_decode_prog_dc, dim3((uint32_t)n), dim3(kThreads), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : hip_fail(e, "progressive decode launch");
}

int mdct_jpegdec_prog_decode(const mdct_jpegdec_scan *desc, int ss, int se, const mdct_jpegdec_tables *tables, const uint8_t *scan,
                             size_t scan_len, const uint64_t *interval_offsets, uint32_t *interval_status, void *stream)
{
  return mdct_jpegdec_prog_decode_approx(desc, ss, se, 0, 0, tables, scan, scan_len, interval_offsets, interval_status, stream);
}

} // extern "C"
