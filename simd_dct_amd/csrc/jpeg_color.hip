// jpeg_color.hip -- decoded JPEG component planes -> 8-bit RGB (include/mdct_jpegcolor.h): libjpeg-turbo's default "fancy" chroma
// upsampling and its integer YCbCr -> RGB, bit for bit.
//
// Built into its own library, libmdct_jpegcolor.so, linked against libmdct_hip.so (whose launch tally counts its launches).  One kernel
// template, k_ycc_rgb<Kind, Planar>: a workgroup is 4 waves on 4 consecutive output rows, a lane owns a run of 16 output pixels of one
// row.  Kind names the sampling the instantiation is specialised for (luma at full size, Cb and Cr alike):
//   kGrey  one plane, copied into R, G and B
//   k444   chroma (1,1)
//   k422   chroma (2,1), chroma width > 2 (fancy horizontal)
//   k420   chroma (2,2), chroma width > 2 (fancy in both directions)
//   kAny   every valid mix of ratios 1..4 per component, and planes taken as R, G, B without conversion
// The specialised kinds load a lane's Y run as two 8-byte loads, and each chroma row and the rows either side it needs as one 8-byte
// (k444: two) load plus the two neighbour bytes, form the sums in registers and store the run as three 16-byte stores (48 interleaved
// bytes, or 16 bytes per plane).  A row whose input or output row start is not aligned for those accesses, the partial run at the
// row's end and every pixel of kAny go through sample(): one pixel at a time, with byte loads and stores.  sample() is the rule itself;
// the vector paths are its specialisation, and the tests hold both against the same checker.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_error.h"
#include "launch_tally.h"
#include "mdct_jpegcolor.h"

namespace mdct
{
namespace jpegcolor
{

enum
{
  kGrey = 0,
  k444 = 1,
  k422 = 2,
  k420 = 3,
  kAny = 4
};

constexpr int kRun = 16;  // output pixels per lane
constexpr int kRows = 4;  // output rows (waves) per workgroup
constexpr int kWG = 64 * kRows;

struct CPlane
{
  const uint8_t *px;
  uint64_t pitch;
  int32_t cw, ch, fh, fv;
};

struct ColorArgs
{
  CPlane p[3];
  uint8_t *out;
  uint64_t pitch, stride;
  int32_t W, H, colour;
};

__device__ __forceinline__ int at(const CPlane &p, int x, int y) { return p.px[(uint64_t)y * p.pitch + (uint32_t)x]; }

// One output sample of component p at image pixel (x, y): libjpeg-turbo's upsampler for the component's ratio (jdsample.c).
// (1,1) copy; (2,1) / (2,2) with cw > 2 and (1,2) at any width: triangle filter, neighbours clamped to the component; all else replicates.
__device__ int sample(const CPlane &p, int x, int y)
{
  if (p.fh == 1 && p.fv == 1)
    return at(p, x, y);
  const bool fancy_h = p.fh == 2 && p.fv <= 2 && p.cw > 2;
  const bool fancy_v = p.fv == 2 && (p.fh == 1 || fancy_h);
  if (!fancy_h && !fancy_v)
    return at(p, x / p.fh, y / p.fv);
  int yy = y, yn = y;
  if (fancy_v)
  {
    yy = y >> 1;
    yn = (y & 1) ? min(yy + 1, p.ch - 1) : max(yy - 1, 0);
  }
  if (!fancy_h)
    return (3 * at(p, x, yy) + at(p, x, yn) + 1 + (y & 1)) >> 2;
  const int xx = x >> 1, xn = (x & 1) ? min(xx + 1, p.cw - 1) : max(xx - 1, 0);
  if (!fancy_v)
    return (3 * at(p, xx, yy) + at(p, xn, yy) + 1 + (x & 1)) >> 2;
  const int s = 3 * at(p, xx, yy) + at(p, xx, yn), sn = 3 * at(p, xn, yy) + at(p, xn, yn);
  return (3 * s + sn + 8 - (x & 1)) >> 4;
}

__device__ __forceinline__ int clamp8(int v) { return min(max(v, 0), 255); }

// jdcolor.c ycc_rgb_convert: (FIX(c) * (C - 128) + ONE_HALF) >> 16, added to Y, clamped.  Every factor fits in 24 signed bits: __mul24
// keeps the products on the full-rate v_mad_i32_i24 (a plain int multiply is the quarter-rate v_mul_lo_u32)
__device__ __forceinline__ void ycc(int y, int cb, int cr, int &r, int &g, int &b)
{
  cb -= 128;
  cr -= 128;
  r = clamp8(y + ((__mul24(91881, cr) + 32768) >> 16));
  g = clamp8(y + ((__mul24(-22554, cb) + __mul24(-46802, cr) + 32768) >> 16));
  b = clamp8(y + ((__mul24(116130, cb) + 32768) >> 16));
}

__device__ __forceinline__ void put(const ColorArgs &a, uint64_t row, int x, int r, int g, int b, bool planar)
{
  if (planar)
  {
    uint8_t *o = a.out + row + (uint32_t)x;
    o[0] = (uint8_t)r;
    o[a.stride] = (uint8_t)g;
    o[2 * a.stride] = (uint8_t)b;
  }
  else
  {
    uint8_t *o = a.out + row + 3 * (uint64_t)x;
    o[0] = (uint8_t)r;
    o[1] = (uint8_t)g;
    o[2] = (uint8_t)b;
  }
}

// pixels [x0, x1) of row y, one at a time
template <int Kind, bool Planar>
__device__ void scalar_run(const ColorArgs &a, int x0, int x1, int y)
{
  const uint64_t row = (uint64_t)y * a.pitch;
  for (int x = x0; x < x1; x++)
  {
    int r, g, b;
    if (Kind == kGrey)
      r = g = b = at(a.p[0], x, y);
    else if (Kind == kAny)
    {
      const int c0 = sample(a.p[0], x, y), c1 = sample(a.p[1], x, y), c2 = sample(a.p[2], x, y);
      if (a.colour == MDCT_JPEGCOLOR_YCBCR)
        ycc(c0, c1, c2, r, g, b);
      else
      {
        r = c0;
        g = c1;
        b = c2;
      }
    }
    else
      ycc(at(a.p[0], x, y), sample(a.p[1], x, y), sample(a.p[2], x, y), r, g, b);
    put(a, row, x, r, g, b, Planar);
  }
}

__device__ __forceinline__ bool aligned(const void *p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

__device__ __forceinline__ void load16(const uint8_t *p, int (&v)[kRun])
{
  const uint2 lo = *reinterpret_cast<const uint2 *>(p), hi = *reinterpret_cast<const uint2 *>(p + 8);
  const uint32_t w[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
  for (int i = 0; i < kRun; i++)
    v[i] = (w[i >> 2] >> (8 * (i & 3))) & 255;
}

// the 8 chroma samples [c0, c0 + 8) of one row and the samples either side (clamped to [0, cw)) -> s[0..9]
__device__ __forceinline__ void load_chroma(const CPlane &p, int c0, int y, int (&s)[10])
{
  const uint8_t *r = p.px + (uint64_t)y * p.pitch;
  const uint2 w = *reinterpret_cast<const uint2 *>(r + c0);
  s[0] = r[max(c0 - 1, 0)];
#pragma unroll
  for (int i = 0; i < 8; i++)
    s[1 + i] = ((i < 4 ? w.x : w.y) >> (8 * (i & 3))) & 255;
  s[9] = r[min(c0 + 8, p.cw - 1)];
}

// chroma of output pixels [x0, x0 + 16): horizontal triangle filter over column values s (row sums for k420), bias / shift per Kind
template <int Kind>
__device__ __forceinline__ void fancy_h(const int (&s)[10], int (&c)[kRun])
{
  constexpr int be = Kind == k420 ? 8 : 1, bo = Kind == k420 ? 7 : 2, sh = Kind == k420 ? 4 : 2;
#pragma unroll
  for (int i = 0; i < 8; i++)
  {
    c[2 * i] = (3 * s[1 + i] + s[i] + be) >> sh;
    c[2 * i + 1] = (3 * s[1 + i] + s[2 + i] + bo) >> sh;
  }
}

template <int Kind>
__device__ __forceinline__ void chroma_run(const CPlane &p, int x0, int y, int (&c)[kRun])
{
  if (Kind == k444)
    load16(p.px + (uint64_t)y * p.pitch + (uint32_t)x0, c);
  else if (Kind == k422)
  {
    int s[10];
    load_chroma(p, x0 >> 1, y, s);
    fancy_h<Kind>(s, c);
  }
  else
  {
    const int yy = y >> 1, yn = (y & 1) ? min(yy + 1, p.ch - 1) : max(yy - 1, 0);
    int s[10], t[10];
    load_chroma(p, x0 >> 1, yy, s);
    load_chroma(p, x0 >> 1, yn, t);
#pragma unroll
    for (int i = 0; i < 10; i++)
      s[i] = 3 * s[i] + t[i];
    fancy_h<Kind>(s, c);
  }
}

__device__ __forceinline__ uint32_t pack4(int a, int b, int c, int d) { return (uint32_t)a | (uint32_t)b << 8 | (uint32_t)c << 16 | (uint32_t)d << 24; }

__device__ __forceinline__ void store16(uint8_t *o, const int (&v)[kRun])
{
  *reinterpret_cast<uint4 *>(o) = make_uint4(pack4(v[0], v[1], v[2], v[3]), pack4(v[4], v[5], v[6], v[7]), pack4(v[8], v[9], v[10], v[11]),
                                             pack4(v[12], v[13], v[14], v[15]));
}

// byte j of the lane's 48 interleaved bytes
__device__ __forceinline__ int rgb_byte(const int (&r)[kRun], const int (&g)[kRun], const int (&b)[kRun], int j)
{
  const int i = j / 3, k = j % 3;
  return k == 0 ? r[i] : k == 1 ? g[i] : b[i];
}

template <int Kind, bool Planar>
__global__ __launch_bounds__(kWG) void k_ycc_rgb(ColorArgs a)
{
  const int y = (int)blockIdx.y * kRows + (int)(threadIdx.x >> 6);
  const int x0 = ((int)blockIdx.x * 64 + (int)(threadIdx.x & 63)) * kRun;
  if (y >= a.H || x0 >= a.W)
    return;
  const int x1 = min(x0 + kRun, a.W);
  uint8_t *orow = a.out + (uint64_t)y * a.pitch;
  bool vec = Kind != kAny && x1 - x0 == kRun && aligned(orow, 16) && (!Planar || (a.stride & 15) == 0);
  const uint8_t *yrow = a.p[0].px + (uint64_t)y * a.p[0].pitch;
  vec = vec && aligned(yrow, 8);
  if (Kind != kGrey && Kind != kAny)
  {
    // every chroma row the run reads: k420 reads row y / 2 and one row either side
    const int yc = Kind == k420 ? y >> 1 : y;
    for (int c = 1; c < 3 && vec; c++)
    {
      const CPlane &p = a.p[c];
      vec = aligned(p.px + (uint64_t)yc * p.pitch, 8) && (Kind != k420 || aligned(p.px + (uint64_t)max(yc - 1, 0) * p.pitch, 8)) &&
            (Kind != k420 || aligned(p.px + (uint64_t)min(yc + 1, p.ch - 1) * p.pitch, 8));
    }
  }
  if (!vec)
  {
    scalar_run<Kind, Planar>(a, x0, x1, y);
    return;
  }
  int Y[kRun], R[kRun], G[kRun], B[kRun];
  load16(yrow + (uint32_t)x0, Y);
  if (Kind == kGrey)
  {
#pragma unroll
    for (int i = 0; i < kRun; i++)
      R[i] = G[i] = B[i] = Y[i];
  }
  else
  {
    int Cb[kRun], Cr[kRun];
    chroma_run<Kind>(a.p[1], x0, y, Cb);
    chroma_run<Kind>(a.p[2], x0, y, Cr);
#pragma unroll
    for (int i = 0; i < kRun; i++)
      ycc(Y[i], Cb[i], Cr[i], R[i], G[i], B[i]);
  }
  if (Planar)
  {
    store16(orow + (uint32_t)x0, R);
    store16(orow + a.stride + (uint32_t)x0, G);
    store16(orow + 2 * a.stride + (uint32_t)x0, B);
  }
  else
  {
    uint4 *o = reinterpret_cast<uint4 *>(orow + 3 * (uint32_t)x0);
#pragma unroll
    for (int q = 0; q < 3; q++)
    {
      uint32_t w[4];
#pragma unroll
      for (int k = 0; k < 4; k++)
      {
        const int j = 16 * q + 4 * k;
        w[k] = pack4(rgb_byte(R, G, B, j), rgb_byte(R, G, B, j + 1), rgb_byte(R, G, B, j + 2), rgb_byte(R, G, B, j + 3));
      }
      o[q] = make_uint4(w[0], w[1], w[2], w[3]);
    }
  }
}

} // namespace jpegcolor
} // namespace mdct

using namespace mdct::jpegcolor;

namespace
{

bool overlaps(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

// the instantiation for this call: the specialised kinds need luma at full size and Cb, Cr alike (422 / 420: wider than 2 samples)
int pick_kind(const mdct_jpegcolor_plane *pl, int n, int colour, const int (&fh)[3], const int (&fv)[3])
{
  if (n == 1)
    return kGrey;
  if (colour != MDCT_JPEGCOLOR_YCBCR || fh[0] != 1 || fv[0] != 1 || fh[1] != fh[2] || fv[1] != fv[2])
    return kAny;
  if (fh[1] == 1 && fv[1] == 1)
    return k444;
  if (fh[1] == 2 && fv[1] == 1 && pl[1].width > 2)
    return k422;
  if (fh[1] == 2 && fv[1] == 2 && pl[1].width > 2)
    return k420;
  return kAny;
}

template <bool Planar>
void launch(int kind, dim3 grid, hipStream_t s, const ColorArgs &a)
{
  switch (kind)
  {
  case kGrey: MDCT_LAUNCH((k_ycc_rgb<kGrey, Planar>), grid, dim3(kWG), 0, s, a); break;
  case k444: MDCT_LAUNCH((k_ycc_rgb<k444, Planar>), grid, dim3(kWG), 0, s, a); break;
  case k422: MDCT_LAUNCH((k_ycc_rgb<k422, Planar>), grid, dim3(kWG), 0, s, a); break;
  case k420: MDCT_LAUNCH((k_ycc_rgb<k420, Planar>), grid, dim3(kWG), 0, s, a); break;
  default: MDCT_LAUNCH((k_ycc_rgb<kAny, Planar>), grid, dim3(kWG), 0, s, a); break;
  }
}

} // namespace

extern "C" {

const char *mdct_jpegcolor_last_error(void) { return g_err; }

int mdct_jpegcolor_to_rgb(const mdct_jpegcolor_plane *planes, int n_planes, size_t width, size_t height, int colour, int layout,
                          uint8_t *out, size_t out_pitch, size_t out_plane_stride, void *stream)
{
  if (!planes || !out)
    return fail(MDCT_INVALID_PARAMETER, "null planes / out");
  if (n_planes != 1 && n_planes != 3)
    return fail(MDCT_INVALID_PARAMETER, "%d planes (1 or 3)", n_planes);
  if (colour != MDCT_JPEGCOLOR_YCBCR && colour != MDCT_JPEGCOLOR_RGB && colour != MDCT_JPEGCOLOR_GREY)
    return fail(MDCT_INVALID_PARAMETER, "colour %d (YCBCR 0, RGB 1, GREY 2)", colour);
  if ((colour == MDCT_JPEGCOLOR_GREY) != (n_planes == 1))
    return fail(MDCT_INVALID_PARAMETER, "colour %d with %d planes (GREY takes one, YCBCR / RGB three)", colour, n_planes);
  if (layout != MDCT_JPEGCOLOR_HWC && layout != MDCT_JPEGCOLOR_CHW)
    return fail(MDCT_INVALID_PARAMETER, "layout %d (HWC 0, CHW 1)", layout);
  if (width < 1 || width > 65535 || height < 1 || height > 65535)
    return fail(MDCT_INVALID_PARAMETER, "image %zux%zu (1..65535 each way)", width, height);
  int hmax = 0, vmax = 0;
  for (int c = 0; c < n_planes; c++)
  {
    if (!planes[c].px)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: null pointer", c);
    if (planes[c].h < 1 || planes[c].h > 4 || planes[c].v < 1 || planes[c].v > 4)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: sampling factors %dx%d (1..4)", c, planes[c].h, planes[c].v);
    hmax = planes[c].h > hmax ? planes[c].h : hmax;
    vmax = planes[c].v > vmax ? planes[c].v : vmax;
  }
  const size_t row_bytes = layout == MDCT_JPEGCOLOR_HWC ? 3 * width : width;
  if (out_pitch < row_bytes)
    return fail(MDCT_INVALID_PARAMETER, "output pitch %zu < %zu bytes per row", out_pitch, row_bytes);
  const size_t plane_span = (height - 1) * out_pitch + row_bytes;
  if (layout == MDCT_JPEGCOLOR_CHW && out_plane_stride < plane_span)
    return fail(MDCT_INVALID_PARAMETER, "output plane stride %zu < %zu bytes per plane", out_plane_stride, plane_span);
  const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (layout == MDCT_JPEGCOLOR_CHW ? 2 * out_plane_stride : 0) + plane_span;
  ColorArgs a;
  int fh[3] = {1, 1, 1}, fv[3] = {1, 1, 1};
  for (int c = 0; c < n_planes; c++)
  {
    const mdct_jpegcolor_plane &p = planes[c];
    if (hmax % p.h || vmax % p.v)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: fractional sampling ratio %d/%d x %d/%d", c, hmax, p.h, vmax, p.v);
    fh[c] = hmax / p.h;
    fv[c] = vmax / p.v;
    const size_t cw = (width * p.h + hmax - 1) / hmax, ch = (height * p.v + vmax - 1) / vmax;
    if (p.width != cw || p.height != ch)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: %zux%zu, the component of a %zux%zu image at %dx%d of %dx%d is %zux%zu", c, p.width, p.height,
                  width, height, p.h, p.v, hmax, vmax, cw, ch);
    if (p.pitch < p.width)
      return fail(MDCT_INVALID_PARAMETER, "plane %d: pitch %zu < width %zu", c, p.pitch, p.width);
    const uintptr_t i0 = (uintptr_t)p.px, i1 = i0 + (p.height - 1) * p.pitch + p.width;
    if (overlaps(o0, o1, i0, i1))
      return fail(MDCT_INVALID_PARAMETER, "plane %d overlaps the output", c);
    a.p[c] = CPlane{p.px, p.pitch, (int32_t)cw, (int32_t)ch, fh[c], fv[c]};
  }
  for (int c = n_planes; c < 3; c++)
    a.p[c] = a.p[0];
  a.out = out;
  a.pitch = out_pitch;
  a.stride = layout == MDCT_JPEGCOLOR_CHW ? out_plane_stride : 0;
  a.W = (int32_t)width;
  a.H = (int32_t)height;
  a.colour = colour;
  const int kind = pick_kind(planes, n_planes, colour, fh, fv);
  const dim3 grid((unsigned)((width + 64 * kRun - 1) / (64 * kRun)), (unsigned)((height + kRows - 1) / kRows));
  if (layout == MDCT_JPEGCOLOR_CHW)
    launch<true>(kind, grid, (hipStream_t)stream, a);
  else
    launch<false>(kind, grid, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MDCT_SUCCESS : fail(MDCT_NOT_SUPPORTED, "launch: %s", hipGetErrorString(e));
}

} // extern "C"
