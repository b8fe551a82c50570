// jpeg_idct_scaled.hip -- quantised JPEG coefficient planes -> 8-bit planes at 1/2, 1/4 or 1/8 size (include/mdct_jpegscale.h):
// libjpeg-turbo's reduced-size inverse (jidctred.c), the box mean of the mathematical IDCT.
//
// Built into its own library, libmdct_jpegscale.so, linked against libmdct_hip.so (whose launch tally counts its launches).  One kernel
// template, k_idct_scaled<Mix>: Mix = 4, 2, 1 when every plane of the call has that n, 0 when they differ (each workgroup then
// branches on its plane's n, uniformly).  A workgroup is 4 waves; a wave takes 64 * K consecutive blocks of one block row of one
// plane, a lane K = 4 / n consecutive blocks: every lane then owns 4 output bytes per output row, stored as one dword where the address
// allows and byte by byte where it does not (or at the row's end).  A lane loads only the coefficient rows whose column of A_n is not
// zero -- n = 4: rows 0-3, 5-7 (16 bytes each, 1 KiB contiguous per wave and row); n = 2: rows 0, 1, 3, 5, 7; n = 1: the DC term alone
// (2 bytes) -- dequantises, and runs the column and the row pass in float32 registers.  No LDS, no scratch.
//
// Arithmetic: out = A_n Z A_n^T with A_n[i, k] = mean over the group of s_k cos((2x + 1) k pi / 16).  The host hands the table over
// divided by 8 (exact), which turns the DC basis function into 1 and the others into sqrt(8) * A_n[i, k]; the level shift is 128
// added to the dequantised DC term.  Even columns of A_n are symmetric in i and odd ones antisymmetric, so half the rows are computed.
// One v_cvt_pk_u8_f32 per sample rounds to nearest even, saturates to 0..255 and places the byte (tools/probe_cvt_pk_u8.hip).
// tests/jpeg_scaled_checker.py restates these operations in numpy float32, in this order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "host_error.h"
#include "launch_tally.h"
#include "mdct_jpegscale.h"

namespace mdct
{
namespace jpegscale
{

constexpr int kMaxPlanes = 4;
constexpr int kWaves = 4; // units (waves) per workgroup
constexpr int kWG = 64 * kWaves;
constexpr uint32_t kMaxBlocks = 8192;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const float __attribute__((address_space(4))) *QPtr; // a table in the kernel-argument segment: scalar loads

struct SPlane
{
  const int16_t *coef;
  uint8_t *px;
  uint64_t pitch_coef, pitch_px; // elements, bytes
  uint32_t bx, by;
  uint32_t chunks; // waves per block row: ceil(bx / (64 * K))
  uint32_t wg0;    // first workgroup of the plane
  int32_t n;
  uint16_t rx, ry; // n = 1: every sample is written rx x ry times
};

struct ScaledArgs
{
  SPlane p[kMaxPlanes];
  float q[kMaxPlanes][64]; // table / 8, natural order
  float shift;             // 128 or 0
  int32_t n_planes;
};

// sqrt(8) * A_4[i, k], i = 0, 1 (A_4[3 - i, k] = +- A_4[i, k]; k = 2, 6: A_4[1, k] = -A_4[0, k]; k = 4: zero)
constexpr float kA4_01 = 1.28145778f, kA4_02 = 0.923879504f, kA4_03 = 0.449988097f, kA4_05 = -0.300672442f, kA4_06 = -0.382683426f,
                kA4_07 = -0.254897803f;
constexpr float kA4_11 = 0.530797184f, kA4_13 = -1.08636737f, kA4_15 = 0.725887477f, kA4_17 = -0.105582118f;
// sqrt(8) * A_2[0, k] (A_2[1, k] = -A_2[0, k] for odd k; even k > 0: zero)
constexpr float kA2_1 = 0.906127453f, kA2_3 = -0.318189651f, kA2_5 = 0.212607518f, kA2_7 = -0.180239961f;

// one 1-D pass: z[0..7] (z[4] not read) -> four group means
__device__ __forceinline__ void pass4(const float (&z)[8], float (&o)[4])
{
  const float g = kA4_02 * z[2] + kA4_06 * z[6];
  const float e0 = z[0] + g, e1 = z[0] - g;
  const float o0 = ((kA4_01 * z[1] + kA4_03 * z[3]) + kA4_05 * z[5]) + kA4_07 * z[7];
  const float o1 = ((kA4_11 * z[1] + kA4_13 * z[3]) + kA4_15 * z[5]) + kA4_17 * z[7];
  o[0] = e0 + o0;
  o[1] = e1 + o1;
  o[2] = e1 - o1;
  o[3] = e0 - o0;
}

// z[0], z[1], z[3], z[5], z[7] -> two group means
__device__ __forceinline__ void pass2(const float (&z)[8], float (&o)[2])
{
  const float od = ((kA2_1 * z[1] + kA2_3 * z[3]) + kA2_5 * z[5]) + kA2_7 * z[7];
  o[0] = z[0] + od;
  o[1] = z[0] - od;
}

template <int N>
__device__ __forceinline__ void pass(const float (&z)[8], float (&o)[N])
{
  if constexpr (N == 4)
    pass4(z, o);
  else
    pass2(z, o);
}

template <int N>
__device__ __forceinline__ constexpr bool used(int k)
{
  return N == 4 ? k != 4 : (k == 0 || (k & 1));
}

__device__ __forceinline__ float coef_at(const u32x4 &r, int u)
{
  const uint32_t w = r[u >> 1];
  return (float)((u & 1) ? (int32_t)w >> 16 : (int32_t)(int16_t)(w & 0xffffu));
}

// one block, N = 4 or 2: its loaded rows -> N bytes at byte `pos` of each of the N output words
template <int N>
__device__ __forceinline__ void block(const u32x4 (&r)[8], QPtr q, float shift, uint32_t (&w)[N], int pos)
{
  float t[N][8]; // column pass: t[i][u]
#pragma unroll
  for (int u = 0; u < 8; u++)
  {
    if (!used<N>(u))
      continue;
    float z[8], o[N];
#pragma unroll
    for (int v = 0; v < 8; v++)
      z[v] = used<N>(v) ? coef_at(r[v], u) * q[v * 8 + u] : 0.0f;
    if (u == 0)
      z[0] += shift;
    pass<N>(z, o);
#pragma unroll
    for (int i = 0; i < N; i++)
      t[i][u] = o[i];
  }
#pragma unroll
  for (int i = 0; i < N; i++)
  {
#pragma unroll
    for (int u = 0; u < 8; u++)
      if (!used<N>(u))
        t[i][u] = 0.0f;
    float o[N];
    pass<N>(t[i], o);
#pragma unroll
    for (int m = 0; m < N; m++)
      w[i] = __builtin_amdgcn_cvt_pk_u8_f32(o[m], (uint32_t)(pos + m), w[i]);
  }
}

// the low `bytes` (1..4) bytes of w to d
__device__ __forceinline__ void put(uint8_t *d, uint32_t w, uint32_t bytes)
{
  if (bytes == 4 && ((uintptr_t)d & 3) == 0)
  {
    *reinterpret_cast<uint32_t *>(d) = w;
    return;
  }
#pragma unroll
  for (uint32_t i = 0; i < 4; i++)
    if (i < bytes)
      d[i] = (uint8_t)(w >> (8 * i));
}

// the wave's unit of plane p: block row by, blocks [chunk * 64 * K, ...)
template <int N>
__device__ __forceinline__ void unit(const int16_t *coef, uint8_t *px, uint64_t pitch_coef, uint64_t pitch_px, uint32_t bx, QPtr q,
                                     float shift, uint32_t by, uint32_t chunk, uint32_t lane, uint32_t rx, uint32_t ry)
{
  constexpr int K = 4 / N;
  const uint32_t b0 = (chunk * 64 + lane) * K;
  if (b0 >= bx)
    return;
  const uint32_t nb = min((uint32_t)K, bx - b0);
  const int16_t *src = coef + (uint64_t)by * 8 * pitch_coef + (uint64_t)b0 * 8;
  uint32_t w[N];
#pragma unroll
  for (int i = 0; i < N; i++)
    w[i] = 0;
  if constexpr (N == 1)
  {
    // a block past the row's end is the row's last block again (loaded, converted, not stored)
    float z[K];
#pragma unroll
    for (int j = 0; j < K; j++)
      z[j] = (float)__builtin_nontemporal_load(src + 8 * min((uint32_t)j, nb - 1));
#pragma unroll
    for (int j = 0; j < K; j++)
      w[0] = __builtin_amdgcn_cvt_pk_u8_f32(z[j] * q[0] + shift, (uint32_t)j, w[0]);
    if (rx * ry != 1)
    {
      // replicated output (libjpeg's plain upsampling at 1/8, where its triangle filters are off): small planes, byte stores
      for (uint32_t r = 0; r < ry; r++)
      {
        uint8_t *row = px + ((uint64_t)by * ry + r) * pitch_px + (uint64_t)b0 * rx;
        for (uint32_t j = 0; j < nb; j++)
          for (uint32_t k = 0; k < rx; k++)
            row[j * rx + k] = (uint8_t)(w[0] >> (8 * j));
      }
      return;
    }
  }
  else
  {
    u32x4 r[K][8];
#pragma unroll
    for (int j = 0; j < K; j++)
    {
      const int16_t *s = src + 8 * min((uint32_t)j, nb - 1);
#pragma unroll
      for (int v = 0; v < 8; v++)
        if (used<N>(v))
          r[j][v] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(s + (uint64_t)v * pitch_coef));
    }
#pragma unroll
    for (int j = 0; j < K; j++)
      block<N>(r[j], q, shift, w, j * N);
  }
  uint8_t *dst = px + (uint64_t)by * N * pitch_px + (uint64_t)b0 * N;
#pragma unroll
  for (int i = 0; i < N; i++)
    put(dst + (uint64_t)i * pitch_px, w[i], nb * N);
}

typedef const ScaledArgs __attribute__((address_space(4))) *KernArgs;

// The arguments are read through the kernel-argument segment itself (the only parameter, at offset 0): a plane index known only at
// run time then costs scalar loads at a computed offset, where indexing the by-value parameter would copy it to scratch first.
template <int Mix>
__global__ __launch_bounds__(kWG) void k_idct_scaled(ScaledArgs)
{
  KernArgs a = (KernArgs)__builtin_amdgcn_kernarg_segment_ptr();
  const uint32_t wg = blockIdx.x;
  int pi = 0;
#pragma unroll
  for (int k = 1; k < kMaxPlanes; k++)
    if (k < a->n_planes && wg >= a->p[k].wg0)
      pi = k;
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const uint32_t chunks = a->p[pi].chunks, bx = a->p[pi].bx;
  const uint32_t u = (wg - a->p[pi].wg0) * kWaves + wave;
  if (u >= a->p[pi].by * chunks)
    return;
  const uint32_t by = u / chunks, chunk = u - by * chunks;
  const int16_t *coef = a->p[pi].coef;
  uint8_t *px = a->p[pi].px;
  const uint64_t pc = a->p[pi].pitch_coef, pp = a->p[pi].pitch_px;
  QPtr q = a->q[pi];
  const float shift = a->shift;
  const int n = Mix ? Mix : a->p[pi].n;
  if (n == 4)
    unit<4>(coef, px, pc, pp, bx, q, shift, by, chunk, lane, 1, 1);
  else if (n == 2)
    unit<2>(coef, px, pc, pp, bx, q, shift, by, chunk, lane, 1, 1);
  else
    unit<1>(coef, px, pc, pp, bx, q, shift, by, chunk, lane, a->p[pi].rx, a->p[pi].ry);
}

} // namespace jpegscale
} // namespace mdct

using namespace mdct::jpegscale;

namespace
{
bool overlaps(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }
} // namespace

extern "C" {

const char *mdct_jpegscale_last_error(void) { return g_err; }

int mdct_jpegscale_inv_i16_u8(const mdct_jpegscale_plane *planes, int n_planes, int level_shift, void *stream)
{
  if (!planes)
    return fail(MDCT_INVALID_PARAMETER, "null planes");
  if (n_planes < 1 || n_planes > kMaxPlanes)
    return fail(MDCT_INVALID_PARAMETER, "%d planes (1..%d)", n_planes, kMaxPlanes);
  if (level_shift != 0 && level_shift != 1)
    return fail(MDCT_INVALID_PARAMETER, "level_shift %d (0 or 1)", level_shift);
  ScaledArgs a = {};
  uintptr_t in0[kMaxPlanes], in1[kMaxPlanes], out0[kMaxPlanes], out1[kMaxPlanes];
  uint64_t wgs = 0;
  int mix = planes[0].n;
  for (int c = 0; c < n_planes; c++)
  {
    const mdct_jpegscale_plane &p = planes[c];
    if (!p.coef || !p.px)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: null coef / px", c);
    if (p.n != 4 && p.n != 2 && p.n != 1)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: n %d (4, 2 or 1; the full size is mdct_inv_i16_u8_batch)", c, p.n);
    if (p.blocks_x < 1 || p.blocks_x > kMaxBlocks || p.blocks_y < 1 || p.blocks_y > kMaxBlocks)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: %zux%zu blocks (1..%u each way)", c, p.blocks_x, p.blocks_y, kMaxBlocks);
    if (p.pitch_coef < p.blocks_x * 8)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: coefficient pitch %zu < %zu elements per row", c, p.pitch_coef, p.blocks_x * 8);
    if (((uintptr_t)p.coef & 15) || (p.pitch_coef & 7))
      return fail(MDCT_INVALID_PARAMETER, "plane %d: coefficient rows are not 16-byte aligned (pointer %p, pitch %zu elements)", c,
                  (const void *)p.coef, p.pitch_coef);
    if (p.rep_x < 0 || p.rep_x > 4 || p.rep_y < 0 || p.rep_y > 4)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: replication %dx%d (1..4 each way, 0 for 1)", c, p.rep_x, p.rep_y);
    const size_t rx = p.rep_x ? p.rep_x : 1, ry = p.rep_y ? p.rep_y : 1;
    if (p.n != 1 && rx * ry != 1)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: replication %zux%zu with n %d (n = 1 only)", c, rx, ry, p.n);
    const size_t row_bytes = p.blocks_x * (size_t)p.n * rx, rows = p.blocks_y * (size_t)p.n * ry;
    if (p.pitch_px < row_bytes)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: output pitch %zu < %zu bytes per row", c, p.pitch_px, row_bytes);
    for (int i = 0; i < 64; i++)
    {
      const float l = p.lut ? p.lut[i] : 1.0f;
      a.q[c][i] = l * 0.125f;
      if (!isfinite(l) || a.q[c][i] == 0.0f)
        return fail(MDCT_INVALID_PARAMETER, "plane %d: table entry %d is %g (finite and non-zero)", c, i, (double)l);
    }
    in0[c] = (uintptr_t)p.coef;
    in1[c] = in0[c] + 2 * ((p.blocks_y * 8 - 1) * p.pitch_coef + p.blocks_x * 8);
    out0[c] = (uintptr_t)p.px;
    out1[c] = out0[c] + (rows - 1) * p.pitch_px + row_bytes;
    const uint32_t per_wave = 64 * (4 / p.n);
    const uint32_t chunks = (uint32_t)((p.blocks_x + per_wave - 1) / per_wave);
    a.p[c] = SPlane{p.coef, p.px, p.pitch_coef, p.pitch_px, (uint32_t)p.blocks_x, (uint32_t)p.blocks_y, chunks, (uint32_t)wgs, p.n, (uint16_t)rx, (uint16_t)ry};
    wgs += ((uint64_t)p.blocks_y * chunks + kWaves - 1) / kWaves;
    if (p.n != mix)
      mix = 0;
  }
  for (int c = 0; c < n_planes; c++)
    for (int d = 0; d < n_planes; d++)
      if (overlaps(out0[c], out1[c], in0[d], in1[d]))
        return fail(MDCT_INVALID_PARAMETER, "the output of plane %d overlaps the coefficients of plane %d", c, d);
  a.shift = level_shift ? 128.0f : 0.0f;
  a.n_planes = n_planes;
  const dim3 grid((unsigned)wgs);
  hipStream_t s = (hipStream_t)stream;
  switch (mix)
  {
  case 4: MDCT_LAUNCH((k_idct_scaled<4>), grid, dim3(kWG), 0, s, a); break;
  case 2: MDCT_LAUNCH((k_idct_scaled<2>), grid, dim3(kWG), 0, s, a); break;
  case 1: MDCT_LAUNCH((k_idct_scaled<1>), grid, dim3(kWG), 0, s, a); break;
  default: MDCT_LAUNCH((k_idct_scaled<0>), grid, dim3(kWG), 0, s, a); break;
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : fail(MDCT_NOT_SUPPORTED, "launch: %s", hipGetErrorString(e));
}

} // extern "C"
