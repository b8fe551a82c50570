// rgb_ycc.h -- the body of the JPEG encoders' front kernels: an 8-bit RGB or grey image -> the padded component planes
// (libjpeg-turbo's integer RGB -> YCbCr, jccolor.c; its chroma downsampling, jcsample.c; edge padding), and the
// host checks of an image and its planes.  One text for k_rgb_ycc (jpeg_encode_color.hip: one image, the record is the kernel's
// argument) and k_batch_rgb_ycc (jpeg_encode_batch.hip: a flat grid over the tiles of many images, the record read from global memory).
//
// rgb_ycc_tile<Kind, Planar> is one workgroup's tile: 4 waves; each wave owns one row group (the fv luma rows and the one chroma row
// they make: 4:2:0 reads every input row once), and a lane owns a run of 16 luma columns of it.  Kind names the sampling:
//   kGrey  one plane, copied (the layout plays no part: one instantiation)
//   k444   chroma (1,1) of luma
//   k422   chroma (2,1): 16 Y and 8 Cb, 8 Cr per lane and row
//   k420   chroma (2,2): 2 x 16 Y and 8 Cb, 8 Cr per lane
// Planar selects the CHW input (three planes: a lane loads 16 bytes of each, 1 KiB per wave and instruction).  HWC input is staged
// through LDS: the wave loads its 3 KiB of each row as three 16-byte loads per lane (1 KiB per instruction, contiguous), and each
// lane reads its 48 bytes back as three ds_read_b128 at a lane stride of 12 dwords -- 3 is coprime to the 16 slots of a bank row, so
// every 16-lane group of ds_read_b128 hits 16 distinct slots (conflict-free, cdna_hip_programming.md section 2).
// A run whose 16 pixels are not all inside the image, a row group that reaches past the image's last row, and rows whose starts are not
// aligned for those accesses go through sample(): one output sample at a time, with byte loads.  sample() is the rule itself; the
// vector path is its specialisation, and the tests hold both against the same checker.
// Include after host_error.h: check_rgb_image leaves its message through that translation unit's fail().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mdct_jpegenc.h"

namespace mdct
{
namespace jpegenc
{

enum
{
  kGrey = 0,
  k444 = 1,
  k422 = 2,
  k420 = 3
};

constexpr int kRun = 16;  // luma columns per lane
constexpr int kRows = 4;  // row groups (waves) per workgroup
constexpr int kWG = 64 * kRows;
constexpr int kRowSlots = 64 * 3; // 16-byte LDS slots of one wave's HWC row: 64 lanes x 48 bytes

struct EPlane
{
  uint8_t *px;
  uint64_t pitch;
  int32_t pw, ph; // padded size
  int32_t cw, ch; // true size
};

struct EncArgs
{
  const uint8_t *in;
  uint64_t pitch, stride;
  EPlane p[3];
  int32_t W, H;
  int32_t X, G; // luma columns and row groups the grid covers
};

template <int Kind> constexpr int kFh = (Kind == k422 || Kind == k420) ? 2 : 1;
template <int Kind> constexpr int kFv = Kind == k420 ? 2 : 1;
// 16-byte LDS slots a workgroup stages its HWC rows in (the other forms stage nothing)
template <int Kind, bool Planar> constexpr int kStageSlots = (!Planar && Kind != kGrey) ? kRows * kFv<Kind> * kRowSlots : 1;

// jccolor.c rgb_ycc_convert.  The products of 16-bit constants and 8-bit samples fit 24 signed bits: __mul24 keeps them on the
// full-rate v_mad_i32_i24 (a plain int multiply is the quarter-rate v_mul_lo_u32).  Every sum is >= 0, so >> is exact.
__device__ __forceinline__ int to_y(int r, int g, int b) { return (__mul24(19595, r) + __mul24(38470, g) + __mul24(7471, b) + 32768) >> 16; }
__device__ __forceinline__ int to_cb(int r, int g, int b) { return (__mul24(-11059, r) + __mul24(-21709, g) + (b << 15) + (128 << 16) + 32767) >> 16; }
__device__ __forceinline__ int to_cr(int r, int g, int b) { return ((r << 15) + __mul24(-27439, g) + __mul24(-5329, b) + (128 << 16) + 32767) >> 16; }

// input channel c at image pixel (x, y), both clamped into the image (libjpeg's right- and bottom-edge replication)
template <int Kind, bool Planar>
__device__ __forceinline__ int in_px(const EncArgs &a, int c, int x, int y)
{
  x = min(x, a.W - 1);
  y = min(y, a.H - 1);
  const uint64_t row = (uint64_t)y * a.pitch;
  if (Kind == kGrey)
    return a.in[row + (uint32_t)x];
  if (Planar)
    return a.in[(uint64_t)c * a.stride + row + (uint32_t)x];
  return a.in[row + 3 * (uint64_t)x + c];
}

// component k (0 Y, 1 Cb, 2 Cr) at full resolution
template <int Kind, bool Planar>
__device__ int full(const EncArgs &a, int k, int x, int y)
{
  if (Kind == kGrey)
    return in_px<Kind, Planar>(a, 0, x, y);
  const int r = in_px<Kind, Planar>(a, 0, x, y), g = in_px<Kind, Planar>(a, 1, x, y), b = in_px<Kind, Planar>(a, 2, x, y);
  return k == 0 ? to_y(r, g, b) : k == 1 ? to_cb(r, g, b) : to_cr(r, g, b);
}

// sample (x, y) of plane k: clamped to the component's true size (padding), then downsampled (jcsample.c h2v1 / h2v2)
template <int Kind, bool Planar>
__device__ int sample(const EncArgs &a, int k, int x, int y)
{
  const EPlane &p = a.p[k];
  x = min(x, p.cw - 1);
  y = min(y, p.ch - 1);
  if (k == 0 || Kind == k444 || Kind == kGrey)
    return full<Kind, Planar>(a, k, x, y);
  if (Kind == k422)
    return (full<Kind, Planar>(a, k, 2 * x, y) + full<Kind, Planar>(a, k, 2 * x + 1, y) + (x & 1)) >> 1;
  return (full<Kind, Planar>(a, k, 2 * x, 2 * y) + full<Kind, Planar>(a, k, 2 * x + 1, 2 * y) + full<Kind, Planar>(a, k, 2 * x, 2 * y + 1) +
          full<Kind, Planar>(a, k, 2 * x + 1, 2 * y + 1) + 1 + (x & 1)) >>
         2;
}

// every sample of row group g in the lane's columns, one at a time
template <int Kind, bool Planar>
__device__ void scalar_group(const EncArgs &a, int x0, int g)
{
  constexpr int fh = kFh<Kind>, fv = kFv<Kind>;
  const int np = Kind == kGrey ? 1 : 3;
  for (int k = 0; k < np; k++)
  {
    const EPlane &p = a.p[k];
    const int sh = k == 0 ? 1 : fh, rows = k == 0 ? fv : 1; // luma columns per sample, plane rows per group
    const int c0 = x0 / sh, c1 = min(c0 + kRun / sh, p.pw);
    for (int r = 0; r < rows; r++)
    {
      const int y = g * rows + r;
      if (y >= p.ph)
        break;
      uint8_t *o = p.px + (uint64_t)y * p.pitch;
      for (int x = c0; x < c1; x++)
        o[x] = (uint8_t)sample<Kind, Planar>(a, k, x, y);
    }
  }
}

__device__ __forceinline__ bool aligned(const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

__device__ __forceinline__ int byte_at(const uint32_t *w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 255; }

__device__ __forceinline__ uint32_t pack4(int a, int b, int c, int d) { return (uint32_t)a | (uint32_t)b << 8 | (uint32_t)c << 16 | (uint32_t)d << 24; }

__device__ __forceinline__ void store16(uint8_t *o, const int *v)
{
  *reinterpret_cast<uint4 *>(o) = make_uint4(pack4(v[0], v[1], v[2], v[3]), pack4(v[4], v[5], v[6], v[7]), pack4(v[8], v[9], v[10], v[11]),
                                             pack4(v[12], v[13], v[14], v[15]));
}

__device__ __forceinline__ void store8(uint8_t *o, const int *v)
{
  *reinterpret_cast<uint2 *>(o) = make_uint2(pack4(v[0], v[1], v[2], v[3]), pack4(v[4], v[5], v[6], v[7]));
}

__device__ __forceinline__ void unpack16(const uint4 &q, int *v)
{
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < kRun; i++)
    v[i] = byte_at(w, i);
}

// the start of every row the vector path of group g reads or writes is aligned for its accesses (wave-uniform)
template <int Kind, bool Planar>
__device__ bool rows_aligned(const EncArgs &a, int g)
{
  constexpr int fv = kFv<Kind>;
  bool ok = true;
#pragma unroll
  for (int r = 0; r < fv; r++)
  {
    const uint64_t row = (uint64_t)(g * fv + r) * a.pitch;
    ok = ok && aligned(a.in + row, 16) && aligned(a.p[0].px + (uint64_t)(g * fv + r) * a.p[0].pitch, 16);
    if (Planar && Kind != kGrey)
      ok = ok && aligned(a.in + a.stride + row, 16) && aligned(a.in + 2 * a.stride + row, 16);
  }
  if (Kind != kGrey)
    for (int k = 1; k < 3; k++)
      ok = ok && aligned(a.p[k].px + (uint64_t)g * a.p[k].pitch, Kind == k444 ? 16 : 8);
  return ok;
}

// The tile (bx, by) of image a: 64 * kRun luma columns from bx * 64 * kRun, kRows row groups from by * kRows.  The whole workgroup
// (kWG threads) calls it with the same a, bx and by (there is a barrier inside); lds: kStageSlots<Kind, Planar> slots.
template <int Kind, bool Planar>
__device__ __forceinline__ void rgb_ycc_tile(const EncArgs &a, int bx, int by, uint4 *lds)
{
  constexpr int fh = kFh<Kind>, fv = kFv<Kind>;
  constexpr bool staged = !Planar && Kind != kGrey;
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const int g = by * kRows + wave;
  const int xw = bx * 64 * kRun, x0 = xw + lane * kRun;
  // the group's luma rows all inside the image (then g < G, and every plane row the group writes exists)
  const bool vec_rows = g * fv + fv <= a.H && rows_aligned<Kind, Planar>(a, g);
  if (staged)
  {
    if (vec_rows)
    {
      const int n = 3 * (a.W - xw); // bytes of the row from the wave's first pixel on
#pragma unroll
      for (int r = 0; r < fv; r++)
      {
        const uint8_t *row = a.in + (uint64_t)(g * fv + r) * a.pitch + 3 * (uint32_t)xw;
#pragma unroll
        for (int q = 0; q < 3; q++)
        {
          const int s = lane + 64 * q;
          if (16 * s + 16 <= n)
            lds[(wave * fv + r) * kRowSlots + s] = *reinterpret_cast<const uint4 *>(row + 16 * s);
        }
      }
    }
    __syncthreads();
  }
  if (g >= a.G || x0 >= a.X)
    return;
  if (!vec_rows || x0 + kRun > a.W)
  {
    scalar_group<Kind, Planar>(a, x0, g);
    return;
  }
  int cb[kRun], cr[kRun];
#pragma unroll
  for (int r = 0; r < fv; r++)
  {
    const uint64_t row = (uint64_t)(g * fv + r) * a.pitch;
    int R[kRun], G[kRun], B[kRun], Y[kRun];
    if (Kind == kGrey)
      unpack16(*reinterpret_cast<const uint4 *>(a.in + row + (uint32_t)x0), Y);
    else
    {
      if (Planar)
      {
        unpack16(*reinterpret_cast<const uint4 *>(a.in + row + (uint32_t)x0), R);
        unpack16(*reinterpret_cast<const uint4 *>(a.in + a.stride + row + (uint32_t)x0), G);
        unpack16(*reinterpret_cast<const uint4 *>(a.in + 2 * a.stride + row + (uint32_t)x0), B);
      }
      else
      {
        const uint4 *s = lds + (wave * fv + r) * kRowSlots + 3 * lane;
        const uint4 q0 = s[0], q1 = s[1], q2 = s[2];
        const uint32_t w[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
#pragma unroll
        for (int i = 0; i < kRun; i++)
        {
          R[i] = byte_at(w, 3 * i);
          G[i] = byte_at(w, 3 * i + 1);
          B[i] = byte_at(w, 3 * i + 2);
        }
      }
#pragma unroll
      for (int i = 0; i < kRun; i++)
      {
        Y[i] = to_y(R[i], G[i], B[i]);
        const int u = to_cb(R[i], G[i], B[i]), v = to_cr(R[i], G[i], B[i]);
        if (fh == 2)
        { // pair sums (4:2:2) or the upper row's pair sums, completed by the lower row (4:2:0)
          if (i & 1)
          {
            cb[i >> 1] += u;
            cr[i >> 1] += v;
          }
          else if (r == 0)
          {
            cb[i >> 1] = u;
            cr[i >> 1] = v;
          }
          else
          {
            cb[i >> 1] += u;
            cr[i >> 1] += v;
          }
        }
        else
        {
          cb[i] = u;
          cr[i] = v;
        }
      }
    }
    store16(a.p[0].px + (uint64_t)(g * fv + r) * a.p[0].pitch + (uint32_t)x0, Y);
  }
  if (Kind == kGrey)
    return;
  uint8_t *ob = a.p[1].px + (uint64_t)g * a.p[1].pitch + (uint32_t)(x0 / fh), *orr = a.p[2].px + (uint64_t)g * a.p[2].pitch + (uint32_t)(x0 / fh);
  if (fh == 1)
  {
    store16(ob, cb);
    store16(orr, cr);
    return;
  }
  // x0 / 2 is even, so output column i of the run has the parity of i
#pragma unroll
  for (int i = 0; i < kRun / 2; i++)
  {
    if (Kind == k422)
    {
      cb[i] = (cb[i] + (i & 1)) >> 1;
      cr[i] = (cr[i] + (i & 1)) >> 1;
    }
    else
    {
      cb[i] = (cb[i] + 1 + (i & 1)) >> 2;
      cr[i] = (cr[i] + 1 + (i & 1)) >> 2;
    }
  }
  store8(ob, cb);
  store8(orr, cr);
}

} // namespace jpegenc
} // namespace mdct

namespace
{

[[maybe_unused]] bool overlaps(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

// The host checks of mdct_jpegenc_from_rgb (include/mdct_jpegenc.h), with its messages; on success a is the kernels' record of the
// image, *kind its sampling and *planar whether the input is CHW.
[[maybe_unused]] int check_rgb_image(const uint8_t *in, size_t in_pitch, size_t in_plane_stride, size_t width, size_t height, int colour, int layout,
                                     const mdct_jpegenc_plane *planes, int n_planes, mdct::jpegenc::EncArgs &a, int *kind, bool *is_planar)
{
  using namespace mdct::jpegenc;
  if (!in || !planes)
    return fail(MDCT_INVALID_PARAMETER, "null input / planes");
  if (colour != MDCT_JPEGENC_RGB && colour != MDCT_JPEGENC_GREY)
    return fail(MDCT_INVALID_PARAMETER, "colour %d (RGB 0, GREY 1)", colour);
  if (layout != MDCT_JPEGENC_HWC && layout != MDCT_JPEGENC_CHW)
    return fail(MDCT_INVALID_PARAMETER, "layout %d (HWC 0, CHW 1)", layout);
  if (n_planes != (colour == MDCT_JPEGENC_GREY ? 1 : 3))
    return fail(MDCT_INVALID_PARAMETER, "%d planes (GREY takes one, RGB three)", n_planes);
  if (width < 1 || width > 65535 || height < 1 || height > 65535)
    return fail(MDCT_INVALID_PARAMETER, "image %zux%zu (1..65535 each way)", width, height);
  for (int c = 0; c < n_planes; c++)
    if (!planes[c].px)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: null pointer", c);
  *kind = kGrey;
  if (colour == MDCT_JPEGENC_GREY)
  {
    if (planes[0].h != 1 || planes[0].v != 1)
      return fail(MDCT_INVALID_PARAMETER, "grey plane: sampling factors %dx%d (1x1)", planes[0].h, planes[0].v);
  }
  else
  {
    const int h = planes[0].h, v = planes[0].v;
    if (planes[1].h != 1 || planes[1].v != 1 || planes[2].h != 1 || planes[2].v != 1)
      return fail(MDCT_INVALID_PARAMETER, "chroma sampling factors %dx%d / %dx%d (1x1)", planes[1].h, planes[1].v, planes[2].h, planes[2].v);
    if (h == 1 && v == 1)
      *kind = k444;
    else if (h == 2 && v == 1)
      *kind = k422;
    else if (h == 2 && v == 2)
      *kind = k420;
    else
      return fail(MDCT_INVALID_PARAMETER, "luma sampling factors %dx%d (1x1, 2x1 or 2x2)", h, v);
  }
  const int hmax = planes[0].h, vmax = planes[0].v;
  // the input's byte span
  const bool planar = colour == MDCT_JPEGENC_RGB && layout == MDCT_JPEGENC_CHW;
  const size_t row_bytes = colour == MDCT_JPEGENC_RGB && layout == MDCT_JPEGENC_HWC ? 3 * width : width;
  if (in_pitch < row_bytes)
    return fail(MDCT_INVALID_PARAMETER, "input pitch %zu < %zu bytes per row", in_pitch, row_bytes);
  const size_t in_span = (height - 1) * in_pitch + row_bytes;
  if (planar && in_plane_stride < in_span)
    return fail(MDCT_INVALID_PARAMETER, "input plane stride %zu < %zu bytes per plane", in_plane_stride, in_span);
  const uintptr_t i0 = (uintptr_t)in, i1 = i0 + (planar ? 2 * in_plane_stride : 0) + in_span;
  uintptr_t o0[3], o1[3];
  for (int c = 0; c < n_planes; c++)
  {
    const mdct_jpegenc_plane &p = planes[c];
    const size_t cw = (width * p.h + hmax - 1) / hmax, ch = (height * p.v + vmax - 1) / vmax;
    if (p.width % 8 || p.height % 8 || p.width < cw || p.height < ch || p.width > 65536 || p.height > 65536)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: %zux%zu; the component of a %zux%zu image at %dx%d of %dx%d is %zux%zu, padded to multiples of 8 "
                  "(at most 65536)", c, p.width, p.height, width, height, p.h, p.v, hmax, vmax, cw, ch);
    if (p.pitch < p.width)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: pitch %zu < width %zu", c, p.pitch, p.width);
    o0[c] = (uintptr_t)p.px;
    o1[c] = o0[c] + (p.height - 1) * p.pitch + p.width;
    if (overlaps(o0[c], o1[c], i0, i1))
      return fail(MDCT_INVALID_PARAMETER, "plane %d overlaps the input", c);
    for (int d = 0; d < c; d++)
      if (overlaps(o0[c], o1[c], o0[d], o1[d]))
        return fail(MDCT_INVALID_PARAMETER, "planes %d and %d overlap", d, c);
    a.p[c] = EPlane{p.px, p.pitch, (int32_t)p.width, (int32_t)p.height, (int32_t)cw, (int32_t)ch};
  }
  for (int c = n_planes; c < 3; c++)
    a.p[c] = a.p[0];
  a.in = in;
  a.pitch = in_pitch;
  a.stride = planar ? in_plane_stride : 0;
  a.W = (int32_t)width;
  a.H = (int32_t)height;
  // luma columns and row groups that cover every plane: chroma sample (x, y) belongs to luma columns [hmax x, hmax x + hmax) of group y
  a.X = a.p[0].pw;
  a.G = (a.p[0].ph + vmax - 1) / vmax;
  if (n_planes == 3)
    for (int c = 1; c < 3; c++)
    {
      a.X = a.X > a.p[c].pw * hmax ? a.X : a.p[c].pw * hmax;
      a.G = a.G > a.p[c].ph ? a.G : a.p[c].ph;
    }
  *is_planar = planar;
  return MDCT_SUCCESS;
}

} // namespace
