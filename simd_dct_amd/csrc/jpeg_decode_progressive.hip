// jpeg_decode_progressive.hip -- the restart-marked scans of a progressive JPEG with spectral selection only (T.81 Annex G,
// Ah = Al = 0) -> quantised int16 coefficient planes (include/mdct_jpegdec_prog.h).
//
// Built into its own library, libmdct_jpegdec_prog.so, linked against libmdct_jpegdec.so (whose table handle, descriptor and interval
// index it takes) and libmdct_hip.so (whose launch tally counts its launches).
//
//   k_decode_prog_dc   a DC-first scan (ss = se = 0), one workgroup per restart interval
//   k_decode_prog_ac   an AC-band scan (1 <= ss <= se <= 63, one component), one workgroup per restart interval
//
// Both are k_decode's model (jpeg_decode.hip) over another symbol grammar: the interval's stuffed bytes are cut into kThreads
// sub-sequences, lane i decodes its own from a guessed state and on to the first symbol boundary past its end, lane i + 1 decodes again
// while the state it started from differs from that exit, prefix sums over the lanes give every lane its first block (and the DC
// predictors there), and a last pass decodes exactly and writes.  From jpegdec_common.h come the bit reader, the Huffman lookup, the
// sub-sequence cut, the table load and the prefix sum; run, speculate, settle and write_pass are this file's own, because the common
// ones are written around the baseline grammar (DC, then AC to 63, per block) and are not to change under k_decode and k_um_*.
//
// The state between two symbols is (bits past the next sub-sequence's first data byte, k, block in MCU) as in k_decode: k is 0 in a DC
// scan and ss..se in an AC band, the block in MCU is 0 in an AC band.  An end-of-band run is accounted whole where its EOBn token is
// decoded: the lane's block count grows by the run and k returns to ss, so no pending run lives across a symbol boundary, the state
// stays one 32-bit word, and the prefix sum of the block counts is exact.  The write pass jumps over the run's blocks.
// While speculating, an invalid code (skip one bit), a level run or a ZRL past se ends the block instead of stopping the lane, and a
// garbage EOBn is simply counted (k_decode's rule: a stopped lane would serialise the interval).
// There is no zeroing pass: the caller's planes are zero in the band, and only an interval that fails sets the band's positions of the
// blocks behind the failing one back to zero (the lanes behind the error wrote levels of the re-synchronised decode there).
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
};

constexpr uint32_t kMaxCount = 0x7FFFFFFFu; // a lane's block count saturates here (a garbage EOBn adds up to 32767 per symbol)

struct PLane
{
  uint32_t state;  // packed start / exit state: kErr | d << 12 | k << 4 | b
  uint32_t blocks; // blocks completed, end-of-band runs included (saturating)
  int dc[3];       // sum of the DC differences per component
  uint32_t err;    // MDCT_JPEGDEC_* of a decode error (final pass)
  bool finished;   // completed the interval's last block (final pass)
  uint32_t fin;    // status after the last block: OK / LEFTOVER / UNEXPECTED_MARKER
};

// the interval's last block is complete: what follows must be its padding (1-bits to the byte boundary) and nothing else
__device__ __forceinline__ uint32_t after_last_block(Reader &r)
{
  refill(r);
  if (r.dry)
  {
    const uint32_t rem = r.uend - r.u;
    if (rem < 8 && (rem == 0 || (uint32_t)(r.buf >> (64 - rem)) == (1u << rem) - 1u))
      return r.marker ? MDCT_JPEGDEC_UNEXPECTED_MARKER : MDCT_JPEGDEC_OK;
  }
  return MDCT_JPEGDEC_LEFTOVER;
}

// Decode from state `start` until the first symbol boundary at or after the next sub-sequence's start (a lane with a successor), the
// interval's last block (WRITE with a unit budget), or an error.  WRITE: unit0 blocks precede the start; pred = DC predictors there.
template <bool AC, bool WRITE>
__device__ void run(Reader &r, const ProgArgs &a, const DevTables &T, const uint32_t *lcomp, uint32_t start, PLane &out, uint32_t unit0,
                    uint32_t units, uint32_t mcu0, int pred[3], uint64_t cap)
{
  const BlockPlace &g = a.d.g;
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
  uint32_t mx = 0, my = 0;
  int16_t *bp = nullptr;
  uint32_t comp = lcomp[b];
  if (WRITE)
  {
    const uint32_t mcu = mcu0 + unit / g.upm;
    my = mcu / g.mcus_x;
    mx = mcu - my * g.mcus_x;
    bp = block_at(g, mx, my, b, comp, 0);
  }
  for (uint64_t it = 0; it < cap; it++)
  {
    refill(r);
    if (r.uE != kNone && r.u >= r.uE)
    {
      out.state = ((r.u - r.uE) << 12) | (k << 4) | b;
      return;
    }
    uint32_t ended = 0; // blocks this symbol completes
    const int sym = huff(r, T, AC ? a.d.bac[0] : a.d.bdc[b]);
    if (sym < 0)
    {
      out.err = no_code(r);
      if (WRITE || out.err != MDCT_JPEGDEC_BAD_CODE)
        return;
      consume(r, 1); // speculating: resynchronise instead of stopping
      out.err = 0;
      ended = 1;
    }
    else if (!AC)
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
        bp[0] = (int16_t)pred[comp];
      }
      ended = 1;
    }
    else
    {
      if (overrun(r))
      {
        out.err = data_error(r);
        return;
      }
      const uint32_t run_ = (uint32_t)sym >> 4, s = (uint32_t)sym & 15;
      if (s == 0 && run_ == 15) // ZRL
      {
        k += 16;
        if (k > a.se + 1)
        {
          if (WRITE)
          {
            out.err = MDCT_JPEGDEC_COEF_OVERFLOW;
            return;
          }
          k = a.se + 1; // speculating: end the block
        }
        ended = k == a.se + 1;
      }
      else if (s == 0) // EOBn: this block and (1 << n) + extra - 1 further ones
      {
        ended = (1u << run_) + get_bits(r, run_);
        if (overrun(r))
        {
          out.err = data_error(r);
          return;
        }
      }
      else
      {
        k += run_;
        if (k > a.se)
        {
          if (WRITE)
          {
            out.err = MDCT_JPEGDEC_COEF_OVERFLOW;
            return;
          }
          k = a.se; // speculating: keep the bit position, end the block after this level
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
          bp[(size_t)(z >> 3) * g.pitch[comp] + (z & 7)] = (int16_t)v;
        }
        k++;
        ended = k == a.se + 1;
      }
    }
    if (ended)
    {
      k = a.ss;
      if (WRITE && ended > units - unit) // unit < units here; the block of the EOBn is the failing one
      {
        out.err = MDCT_JPEGDEC_EOBRUN_OVERFLOW;
        return;
      }
      out.blocks = out.blocks + ended < kMaxCount ? out.blocks + ended : kMaxCount;
      if (!AC)
      {
        if (++b == g.upm)
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
        if (ended == 1)
        {
          if (b == 0 && ++mx == g.mcus_x)
          {
            mx = 0;
            my++;
          }
        }
        else // AC only (one block per MCU): over the run's blocks
        {
          const uint32_t mcu = mcu0 + unit;
          my = mcu / g.mcus_x;
          mx = mcu - my * g.mcus_x;
        }
        bp = block_at(g, mx, my, b, comp, 0);
      }
    }
  }
  out.err = MDCT_JPEGDEC_OUT_OF_DATA; // not reached: every symbol consumes a bit and the data ends
}

// one speculating decode of the lane's sub-sequence from state `start`; a lane without data publishes no usable exit and counts nothing
template <bool AC>
__device__ __forceinline__ void speculate(const ProgArgs &a, const DevTables &T, const uint32_t *lcomp, const SubLane &q, uint32_t start, PLane &L)
{
  Reader r;
  int dummy[3] = {0, 0, 0};
  L.state = kErr;
  L.blocks = 0;
  L.dc[0] = L.dc[1] = L.dc[2] = 0;
  if (!q.active)
    return;
  reader_init(r, a.d, q.s0, q.end, q.E, q.first);
  run<AC, false>(r, a, T, lcomp, start, L, 0, 0, 0, dummy, q.cap);
}

// lane 0 wants want0, lane i the exit of lane i - 1; a lane whose start differs decodes again, until no start changes (at most nact + 1
// trips: each trip makes one more lane exact).  exit_state: kThreads words of LDS.
template <bool AC>
__device__ __forceinline__ void settle(const ProgArgs &a, const DevTables &T, const uint32_t *lcomp, const SubLane &q, uint32_t want0,
                                       uint32_t &my_start, PLane &L, uint32_t *exit_state)
{
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
      speculate<AC>(a, T, lcomp, q, my_start, L);
      exit_state[threadIdx.x] = L.state;
    }
  }
  wg_sync();
}

// The write pass of a lane with data: the exact decode from `start`.  A decode error goes to *first_err (LDS, kNone before) as
// lane << 8 | code, the smallest winning; the status after the interval's last block to *fin.  Returns the unit the lane stopped in.
template <bool AC>
__device__ __forceinline__ uint32_t write_pass(const ProgArgs &a, const DevTables &T, const uint32_t *lcomp, const SubLane &q, uint32_t start,
                                               uint32_t unit0, uint32_t units, uint32_t mcu0, int pred[3], uint32_t *first_err, uint32_t *fin)
{
  Reader r;
  PLane F;
  reader_init(r, a.d, q.s0, q.end, q.E, q.first);
  run<AC, true>(r, a, T, lcomp, start, F, unit0, units, mcu0, pred, q.cap);
  if (F.err && unit0 < units)
    atomicMin(first_err, ((uint32_t)threadIdx.x << 8) | F.err);
  if (F.finished)
    *fin = F.fin;
  return unit0 + F.blocks;
}

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

template <bool AC>
__device__ __forceinline__ void decode_interval(const ProgArgs &a, DevTables &T, uint32_t *exit_state, uint32_t *lcomp, int *wtot,
                                                uint32_t *first_err, uint32_t *fin_word, uint32_t *fail_unit)
{
  const int tid = threadIdx.x;
  const uint32_t k = blockIdx.x;
  load_tables(a.d, T, lcomp, tid);
  if (tid == 0)
  {
    *first_err = kNone;
    *fin_word = kNone;
  }
  // the interval's data, clamped into the scan whatever the offsets say
  const uint64_t len = a.d.scan_len;
  const bool last = k + 1 == a.d.n_intervals;
  uint64_t s = a.d.off[k];
  const uint64_t next = a.d.off[k + 1];
  uint64_t e = last ? next : (next >= 2 ? next - 2 : 0);
  s = s < len ? s : len;
  e = e < len ? e : len;
  e = e > s ? e : s;
  // T.81 B.1.1.2: 0xFF bytes directly before the interval's RSTm are fill bytes, not data
  if (!last && next <= len)
    for (uint64_t i = 0, n = e - s; i < n && a.d.scan[e - 1] == 0xFF; i++)
      e--;
  const uint64_t sb = (e - s + kThreads - 1) / kThreads;
  const SubLane q = sub_lane(s, e, sb < 8 ? 8 : sb, tid, true);
  const uint32_t mcu0 = k * a.d.restart;
  const uint32_t nmcu = (a.d.total_mcus - mcu0) < a.d.restart ? a.d.total_mcus - mcu0 : a.d.restart;
  const uint32_t units = nmcu * a.d.g.upm;
  wg_sync();

  // ---- synchronisation: lane 0 starts exact (the band's first position of an MCU's first block), the others from the same guess
  PLane L;
  const uint32_t want0 = a.ss << 4;
  uint32_t my_start = want0;
  speculate<AC>(a, T, lcomp, q, my_start, L);
  settle<AC>(a, T, lcomp, q, want0, my_start, L, exit_state);

  // ---- blocks before each lane's start, and the DC predictors there
  const uint32_t unit0 = first_unit(L.blocks, units, wtot);
  int pred[3] = {0, 0, 0};
  if (!AC)
    for (int c = 0; c < 3; c++)
      pred[c] = wg_excl_scan(L.dc[c], wtot);

  // ---- the decode proper
  uint32_t stop = 0;
  if (q.active)
    stop = write_pass<AC>(a, T, lcomp, q, my_start, unit0, units, mcu0, pred, first_err, fin_word);
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
    uint32_t st = *first_err != kNone ? (*first_err & 0xFF) : (*fin_word != kNone ? *fin_word : (uint32_t)MDCT_JPEGDEC_OUT_OF_DATA);
    if (st == MDCT_JPEGDEC_OK && !last)
    {
      // the marker after the interval must be RST(k mod 8)
      const bool ok = next >= 2 && next <= len && next - 2 >= s && a.d.scan[next - 2] == 0xFF && a.d.scan[next - 1] == 0xD0 + (k & 7);
      if (!ok)
        st = MDCT_JPEGDEC_UNEXPECTED_MARKER;
    }
    a.d.status[k] = st;
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

int mdct_jpegdec_prog_decode(const mdct_jpegdec_scan *desc, int ss, int se, const mdct_jpegdec_tables *tables, const uint8_t *scan,
                             size_t scan_len, const uint64_t *interval_offsets, uint32_t *interval_status, void *stream)
{
  mdct_jpegdec_scan d;
  size_t n = 0;
  int rc = check_prog(desc, ss, se, d, &n);
  if (rc)
    return rc;
  if (!tables || !interval_offsets || !interval_status || (!scan && scan_len))
    return fail(MDCT_INVALID_PARAMETER, "null tables / scan / offsets / status");
  const bool ac = ss > 0;
  // only the slots of the band's class must be present: the other class counts as present for fill_geometry and is never read
  mdct_jpegdec_tables used = *tables;
  for (int t = 0; t < 4; t++)
    if ((t >= 2) != ac)
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
  if (ac)
    MDCT_LAUNCH(prog::k_decode_prog_ac, dim3((uint32_t)n), dim3(kThreads), 0, (hipStream_t)stream, a);
  else
    MDCT_LAUNCH(prog::k_decode_prog_dc, dim3((uint32_t)n), dim3(kThreads), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : hip_fail(e, "progressive decode launch");
}

} // extern "C"
