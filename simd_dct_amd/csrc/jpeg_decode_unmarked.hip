// jpeg_decode_unmarked.hip -- baseline JPEG scans WITHOUT restart markers -> quantised int16 coefficient planes
// (include/mdct_jpegdec_unmarked.h).
//
// Built into its own library, libmdct_jpegdec_unmarked.so, linked against libmdct_jpegdec.so (whose table handle it accepts) and
// libmdct_hip.so (whose launch tally counts its launches).  A scan without markers is one interval of up to several MB; k_decode's
// sub-sequence synchronisation (jpegdec_common.h: speculate, settle) is lifted one level: the stuffed scan is cut into chunks of kThreads
// sub-sequences of kSubBytes bytes, one workgroup per chunk, and the chunks are synchronised with each other across kernel boundaries only.
//
//   k_um_zero    every block the descriptor names, zeroed with 16-byte stores
//   k_um_sync    one workgroup per chunk: lane 0 of chunk 0 starts exact, lane 0 of every other chunk from a guess (bit 0 of its first
//                byte, DC of the MCU's first block); the lanes synchronise inside the chunk as in k_decode.  Every lane's start and
//                exit state, block count and per-component DC sums go to the workspace, the chunk's totals and its last lane's exit
//                (the state the next chunk's lane 0 must start from) too
//   k_um_round   launched sync_rounds times (round r = 1, 2, ...).  A chunk whose predecessor published (in round r - 1) an exit state
//                other than the start its lane 0 used decodes again: lane 0 from the new start, then every lane whose start changed,
//                from the states kept in the workspace.  A chunk publishes its exit every round (two buffers, by the round's parity)
//                and records the round in the workspace's control word when that exit changed; a round in which the control word
//                shows no change in the previous one returns at once.  After round r, chunks 0..r are exact at the least.
//                A predecessor whose exit is kErr asks for nothing: exact decoding stops with an error (or after the last block)
//                inside it, so the scan's status is settled there and the chunks after it need not be exact
//   k_um_prefix  one workgroup: every chunk's lane-0 start must equal its predecessor's final exit unless that is kErr (else
//                NOT_SYNCHRONISED and no level is written); exclusive prefixes of the chunks' block counts and DC sums.  The chunks
//                from the first one whose start went unchecked that way on write nothing: the scan's first error lies before them
//   k_um_write   one workgroup per chunk: each lane's first block and DC predictors from the chunk's prefix and the lanes' prefix, then
//                the exact decode of its range, writing levels, as k_decode's last pass.  The first error in decoding order, and the
//                number of blocks before it, per chunk
//   k_um_final   one workgroup: the scan's status and block count from the chunks' first errors; after an error, the blocks behind the
//                failing one zeroed again (the lanes behind the error wrote levels of the re-synchronised decode into them)
// No workgroup waits for another inside a launch: every hand-off between chunks crosses a kernel boundary.  Every loop has a bound.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "jpegdec_common.h"
#include "launch_tally.h"
#include "mdct_jpegdec_unmarked.h"

namespace mdct
{
namespace jpegdec
{

constexpr uint32_t kSubBytes = 32;                   // stuffed bytes per sub-sequence (lane)
constexpr uint64_t kChunkBytes = kSubBytes * kThreads; // 8 KiB per workgroup
constexpr uint64_t kMaxScan = 1ull << 28;            // block counts and lane indices stay far inside 32 bits

// control words at the workspace's start
enum
{
  kLastRound = 0, // the last round in which some chunk's published exit changed (k_um_sync: 0)
  kSyncOk = 1,    // k_um_prefix: 1 when every chunk's start matched its predecessor's exit
  kFin = 2,       // k_um_write: status after the scan's last block (kNone: no lane got there)
  kTotal = 3,     // k_um_prefix: blocks counted over the whole scan
  kLoose = 4,     // k_um_prefix: the first chunk whose start was not checked (its predecessor ended in kErr): it and those after it write nothing
  kCtlWords = 16
};

struct UmArgs
{
  DecArgs d;             // scan, tables, block layout (off / status / restart / n_intervals unused)
  uint32_t *status;      // [2]: MDCT_JPEGDEC_*, blocks decoded before the first error
  uint32_t nchunks, units, rounds;
  uint64_t nlanes;       // nchunks * kThreads
  uint32_t *ctl;         // [kCtlWords]
  uint32_t *start, *exit_; // [nlanes] per-lane start / exit state
  int *blocks;           // [nlanes]
  int *dc;               // [3][nlanes]
  int *ctot, *cbase;     // [4][nchunks]: chunk totals (blocks, dc0, dc1, dc2) / their exclusive prefixes
  uint32_t *pub;         // [2][nchunks]: every chunk's last exit state, by round parity
  uint32_t *cerr, *ccnt; // [nchunks]: first error in the chunk (lane << 8 | code, kNone), blocks before it
};

// the chunk's totals (blocks, DC sums) into ctot
__device__ void chunk_totals(const UmArgs &a, uint32_t c, const Lane &L, bool active, int *tot)
{
  if (threadIdx.x < 4)
    tot[threadIdx.x] = 0;
  wg_sync();
  if (active)
  {
    atomicAdd(&tot[0], L.blocks);
    for (int k = 0; k < 3; k++)
      atomicAdd(&tot[1 + k], L.dc[k]);
  }
  wg_sync();
  if (threadIdx.x < 4)
    a.ctot[(size_t)threadIdx.x * a.nchunks + c] = tot[threadIdx.x];
}

__device__ __forceinline__ void store_lane(const UmArgs &a, uint64_t g, uint32_t my_start, const Lane &L, bool active)
{
  a.start[g] = my_start;
  a.exit_[g] = active ? L.state : kErr;
  a.blocks[g] = active ? L.blocks : 0;
  for (int k = 0; k < 3; k++)
    a.dc[(size_t)k * a.nlanes + g] = active ? L.dc[k] : 0;
}

__global__ void __launch_bounds__(kThreads) k_um_zero(UmArgs a)
{
  zero_units<uint64_t>(a.d.g, 0, 0, a.units, (uint64_t)blockIdx.x * kThreads + threadIdx.x, (uint64_t)gridDim.x * kThreads);
}

__global__ void __launch_bounds__(kThreads) k_um_sync(UmArgs a)
{
  __shared__ DevTables T;
  __shared__ uint32_t exit_state[kThreads];
  __shared__ uint32_t lcomp[16];
  __shared__ int tot[4];
  const int tid = threadIdx.x;
  const uint32_t c = blockIdx.x;
  load_tables(a.d, T, lcomp, tid);
  if (c == 0 && tid == 0)
    a.ctl[kLastRound] = 0;
  const SubLane q = sub_lane((uint64_t)c * kChunkBytes, a.d.scan_len, kSubBytes, tid, c == 0); // lane 0 of chunk 0 starts exact
  wg_sync();
  Lane L;
  uint32_t my_start = 0;
  speculate(a.d, Sequential(), T, lcomp, q, my_start, L);
  settle(a.d, Sequential(), T, lcomp, q, 0u, my_start, L, exit_state); // lane 0 keeps its start: exact in chunk 0, the guess elsewhere
  store_lane(a, (uint64_t)c * kThreads + tid, my_start, L, q.active);
  chunk_totals(a, c, L, q.active, tot);
  if (tid == 0)
    a.pub[c] = exit_state[q.nact - 1];
}

__global__ void __launch_bounds__(kThreads) k_um_round(UmArgs a, uint32_t rnd)
{
  __shared__ DevTables T;
  __shared__ uint32_t exit_state[kThreads];
  __shared__ uint32_t lcomp[16];
  __shared__ int tot[4];
  __shared__ uint32_t go, want0;
  const int tid = threadIdx.x;
  const uint32_t c = blockIdx.x;
  const SubLane q = sub_lane((uint64_t)c * kChunkBytes, a.d.scan_len, kSubBytes, tid, c == 0); // lane 0 of chunk 0 starts exact
  const uint64_t g = (uint64_t)c * kThreads + tid, g_last = (uint64_t)c * kThreads + q.nact - 1; // indices among all lanes
  uint32_t *pub_now = a.pub + (size_t)(rnd & 1) * a.nchunks;
  if (tid == 0)
  {
    // rnd - 1 or rnd (a chunk of this round that already recorded a change): the previous round changed something
    go = a.ctl[kLastRound] + 1 >= rnd;
    want0 = c == 0 ? 0u : a.pub[(size_t)((rnd - 1) & 1) * a.nchunks + c - 1];
    if (go && (want0 == kErr || want0 == a.start[(uint64_t)c * kThreads]))
    {
      pub_now[c] = a.exit_[g_last]; // unchanged: republish for this round's parity
      go = 0;
    }
  }
  wg_sync();
  if (!go)
    return;
  load_tables(a.d, T, lcomp, tid);
  uint32_t my_start = a.start[g];
  Lane L;
  L.state = a.exit_[g]; // a lane without data: kErr, no blocks, no DC, as k_um_sync stored them for all nlanes of this scan (store_lane)
  L.blocks = a.blocks[g];
  for (int k = 0; k < 3; k++)
    L.dc[k] = a.dc[(size_t)k * a.nlanes + g];
  const uint32_t old_exit = a.exit_[g_last];
  wg_sync();
  if (settle(a.d, Sequential(), T, lcomp, q, want0, my_start, L, exit_state))
    store_lane(a, g, my_start, L, q.active);
  chunk_totals(a, c, L, q.active, tot);
  if (tid == 0)
  {
    const uint32_t e = exit_state[q.nact - 1];
    pub_now[c] = e;
    if (e != old_exit)
      atomicMax(&a.ctl[kLastRound], rnd);
  }
}

__global__ void __launch_bounds__(1024) k_um_prefix(UmArgs a)
{
  __shared__ int wtot[16];
  __shared__ uint32_t loose;
  const uint32_t *pub = a.pub + (size_t)(a.rounds & 1) * a.nchunks;
  if (threadIdx.x == 0)
    loose = a.nchunks;
  __syncthreads();
  bool bad = false;
  for (uint32_t c = 1 + threadIdx.x; c < a.nchunks; c += 1024)
    if (a.start[(uint64_t)c * kThreads] != pub[c - 1])
    {
      if (pub[c - 1] != kErr)
        bad = true;
      else
        atomicMin(&loose, c);
    }
  const bool ok = !__syncthreads_or(bad);
  const int total = wg1024_excl_prefix(a.ctot, a.cbase, a.nchunks, wtot); // blocks
  for (int k = 1; k < 4; k++)                                             // DC sums
    wg1024_excl_prefix(a.ctot + (size_t)k * a.nchunks, a.cbase + (size_t)k * a.nchunks, a.nchunks, wtot);
  if (threadIdx.x == 0)
  {
    a.ctl[kSyncOk] = ok;
    a.ctl[kFin] = kNone;
    a.ctl[kTotal] = (uint32_t)total;
    a.ctl[kLoose] = loose;
  }
}

__global__ void __launch_bounds__(kThreads) k_um_write(UmArgs a)
{
  __shared__ DevTables T;
  __shared__ uint32_t lcomp[16];
  __shared__ int wtot[kThreads / 64];
  __shared__ uint32_t first_err;
  const int tid = threadIdx.x;
  const uint32_t c = blockIdx.x;
  if (!a.ctl[kSyncOk] || c >= a.ctl[kLoose])
  {
    // a lane behind an unchecked hand-off may hold a block-in-MCU that is not its unit's: it could overwrite an earlier block of the
    // MCU the scan's first error is in.  Those chunks lie after that error, so they decide nothing either.
    if (tid == 0)
      a.cerr[c] = kNone;
    return;
  }
  load_tables(a.d, T, lcomp, tid);
  if (tid == 0)
    first_err = kNone;
  const SubLane q = sub_lane((uint64_t)c * kChunkBytes, a.d.scan_len, kSubBytes, tid, c == 0); // lane 0 of chunk 0 starts exact
  const uint64_t g = (uint64_t)c * kThreads + tid;
  const int nb = q.active ? a.blocks[g] : 0;
  const uint32_t unit0 = (uint32_t)(a.cbase[c] + wg_excl_scan(nb, wtot));
  int pred[3];
  for (int k = 0; k < 3; k++)
    pred[k] = a.cbase[(size_t)(1 + k) * a.nchunks + c] + wg_excl_scan(q.active ? a.dc[(size_t)k * a.nlanes + g] : 0, wtot);
  uint32_t stop = 0;
  if (q.active) // (one lane of the whole scan completes its last block and writes kFin)
    stop = write_pass(a.d, Sequential(), T, lcomp, q, a.start[g], unit0, a.units, 0, pred, &first_err, &a.ctl[kFin]);
  wg_sync();
  const uint32_t fe = first_err;
  if (fe != kNone && (uint32_t)tid == fe >> 8)
    a.ccnt[c] = stop;
  if (tid == 0)
    a.cerr[c] = fe;
}

__global__ void __launch_bounds__(1024) k_um_final(UmArgs a)
{
  __shared__ uint32_t first, zero_from;
  if (threadIdx.x == 0)
  {
    first = kNone;
    zero_from = a.units;
  }
  __syncthreads();
  if (!a.ctl[kSyncOk])
  {
    if (threadIdx.x == 0)
    {
      a.status[0] = MDCT_JPEGDEC_NOT_SYNCHRONISED;
      a.status[1] = 0;
    }
    return;
  }
  uint32_t m = kNone;
  for (uint32_t c = threadIdx.x; c < a.nchunks; c += 1024)
    if (a.cerr[c] != kNone)
    {
      m = c;
      break;
    }
  if (m != kNone)
    atomicMin(&first, m);
  __syncthreads();
  if (threadIdx.x == 0)
  {
    uint32_t st, n;
    if (first != kNone)
    {
      st = a.cerr[first] & 0xFF;
      n = a.ccnt[first];
      zero_from = n + 1;
    }
    else if (a.ctl[kFin] != kNone)
    {
      st = a.ctl[kFin];
      n = a.units;
    }
    else
    {
      st = MDCT_JPEGDEC_OUT_OF_DATA;
      n = a.ctl[kTotal] < a.units ? a.ctl[kTotal] : a.units;
    }
    a.status[0] = st;
    a.status[1] = n;
  }
  __syncthreads();
  // After an error the lanes and chunks behind it wrote levels of the re-synchronised decode into blocks after the failing one (block n):
  // those go back to zero.  Block n keeps the levels decoded before the error.  An error path only: one workgroup is enough.
  const uint32_t z0 = zero_from < a.units ? zero_from : a.units;
  zero_units<uint64_t>(a.d.g, 0, z0, a.units - z0, threadIdx.x, 1024);
}

} // namespace jpegdec
} // namespace mdct

using namespace mdct::jpegdec;

namespace
{
struct Layout
{
  uint64_t nchunks, nlanes;
  size_t start, exit_, blocks, dc, ctot, cbase, pub, cerr, ccnt, bytes; // byte offsets into the workspace
};

Layout layout(size_t scan_len)
{
  Layout l;
  l.nchunks = scan_len ? (scan_len + kChunkBytes - 1) / kChunkBytes : 1;
  l.nlanes = l.nchunks * kThreads;
  size_t p = kCtlWords * 4;
  auto take = [&p](size_t n) {
    const size_t at = p;
    p = (p + n + 255) / 256 * 256;
    return at;
  };
  l.start = take(l.nlanes * 4);
  l.exit_ = take(l.nlanes * 4);
  l.blocks = take(l.nlanes * 4);
  l.dc = take(l.nlanes * 12);
  l.ctot = take(l.nchunks * 16);
  l.cbase = take(l.nchunks * 16);
  l.pub = take(l.nchunks * 8);
  l.cerr = take(l.nchunks * 4);
  l.ccnt = take(l.nchunks * 4);
  l.bytes = p;
  return l;
}

int check_unmarked(const mdct_jpegdec_scan *d, size_t scan_len)
{
  const int rc = check_scan_head(d, false, "restart interval %zu: a scan with restart markers goes to mdct_jpegdec_decode");
  if (rc)
    return rc;
  if (scan_len >= kMaxScan)
    return fail(MDCT_NOT_SUPPORTED, "scan of %zu bytes (less than 2^28)", scan_len);
  return check_components(d);
}
} // namespace

extern "C" {

const char *mdct_jpegdec_unmarked_last_error(void) { return g_err; }

size_t mdct_jpegdec_unmarked_workspace(const mdct_jpegdec_scan *desc, size_t scan_len)
{
  return check_unmarked(desc, scan_len) ? 0 : layout(scan_len).bytes;
}

int mdct_jpegdec_decode_unmarked(const mdct_jpegdec_scan *desc, const mdct_jpegdec_tables *tables, const uint8_t *scan, size_t scan_len,
                                 void *workspace, size_t workspace_bytes, uint32_t *status, int sync_rounds, void *stream)
{
  int rc = check_unmarked(desc, scan_len);
  if (rc)
    return rc;
  if (!tables || !workspace || !status || (!scan && scan_len))
    return fail(MDCT_INVALID_PARAMETER, "null tables / scan / workspace / status");
  if (sync_rounds < 0)
    return fail(MDCT_INVALID_PARAMETER, "sync_rounds %d (>= 0)", sync_rounds);
  const Layout l = layout(scan_len);
  if (workspace_bytes < l.bytes)
    return fail(MDCT_INVALID_PARAMETER, "workspace of %zu bytes, this scan needs %zu", workspace_bytes, l.bytes);
  if ((uintptr_t)workspace & 15)
    return fail(MDCT_INVALID_PARAMETER, "workspace not 16-byte aligned");
  UmArgs a;
  memset(&a, 0, sizeof(a));
  a.d.scan = scan;
  a.d.scan_len = scan_len;
  if ((rc = fill_geometry(desc, tables, a.d)))
    return rc;
  char *w = (char *)workspace;
  a.status = status;
  a.nchunks = (uint32_t)l.nchunks;
  a.nlanes = l.nlanes;
  a.units = a.d.total_mcus * a.d.g.upm;
  a.rounds = l.nchunks > 1 ? (uint32_t)sync_rounds : 0u;
  a.ctl = (uint32_t *)w;
  a.start = (uint32_t *)(w + l.start);
  a.exit_ = (uint32_t *)(w + l.exit_);
  a.blocks = (int *)(w + l.blocks);
  a.dc = (int *)(w + l.dc);
  a.ctot = (int *)(w + l.ctot);
  a.cbase = (int *)(w + l.cbase);
  a.pub = (uint32_t *)(w + l.pub);
  a.cerr = (uint32_t *)(w + l.cerr);
  a.ccnt = (uint32_t *)(w + l.ccnt);
  hipStream_t s = (hipStream_t)stream;
  const uint64_t zwork = (uint64_t)a.units * 8;
  const uint32_t zgrid = (uint32_t)(zwork / kThreads < 8192 ? (zwork + kThreads - 1) / kThreads : 8192);
  MDCT_LAUNCH(k_um_zero, dim3(zgrid), dim3(kThreads), 0, s, a);
  MDCT_LAUNCH(k_um_sync, dim3(a.nchunks), dim3(kThreads), 0, s, a);
  for (uint32_t r = 1; r <= a.rounds; r++)
    MDCT_LAUNCH(k_um_round, dim3(a.nchunks), dim3(kThreads), 0, s, a, r);
  MDCT_LAUNCH(k_um_prefix, dim3(1), dim3(1024), 0, s, a);
  MDCT_LAUNCH(k_um_write, dim3(a.nchunks), dim3(kThreads), 0, s, a);
  MDCT_LAUNCH(k_um_final, dim3(1), dim3(1024), 0, s, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : hip_fail(e, "unmarked decode launch");
}

} // extern "C"
